"""GPU (-m gpu): the grayscale JPEG read (gray=True; csrc/k20_jpeg_gray.hip: k_jpeg_gray8, k_jpeg_gray4, k_jpeg_gray_small<2>, <1>, fed by the
luma-only entropy decode of csrc/host_jpeg.cpp) against the numpy restatement tests/jpeg_gray_ref.py, which test_jpeg_gray_ref.expected()
holds against Pillow's libjpeg-turbo luma-only decode wherever Pillow can decode at that scale.  Exact bytes, through the compact and the
dense transport, at scale 1, 1/2, 1/4 and 1/8."""
import functools

import numpy as np
import pytest
import torch

import jpeg_gray_ref as G
import test_jpeg_crafted as T
from test_jpeg import encode, synth_image
from test_jpeg_gray_host import restart_files
from test_jpeg_gray_ref import SUBS, expected, gray_file, gray_files, photo

pytestmark = pytest.mark.gpu


def assert_gray(ctx, data, d, what="", **kw):
    want = expected(data, d)
    for dense in (False, True):
        got = ctx.imdecode(data, dense=dense, reduce=d, gray=True, **kw)
        assert got.dtype == torch.uint8 and got.dim() == 2 and got.is_cuda
        got = got.cpu().numpy()
        assert got.shape == want.shape, (what, d, dense, got.shape, want.shape)
        assert (got == want).all(), (what, d, dense, int((got != want).sum()))
    return want


@pytest.mark.parametrize("d", G.SCALES)
@pytest.mark.parametrize("sub", SUBS)
def test_gray_sizes_samplings_scales(ctx, sub, d):
    """1x1, 7x5, 8x8, 9x9, 16x16, 17x17, 33x17, 53x37 at qualities 30 and 95: single blocks, partial blocks and MCUs, odd reduced sizes"""
    for what, data in gray_files(sub):
        assert_gray(ctx, data, d, what)


@pytest.mark.parametrize("d", G.SCALES)
def test_gray_restart_intervals(ctx, d):
    for what, data in restart_files():
        assert_gray(ctx, data, d, what)
        assert (ctx.imdecode(data, threads=2, reduce=d, gray=True).cpu().numpy() == expected(data, d)).all(), what


@pytest.mark.parametrize("d", G.SCALES)
def test_gray_wider_than_a_workgroup(ctx, d):
    """more than 32 (S = 8) and 64 (S = 4, 2, 1) blocks across and more than 4 block rows: several workgroups in x and y, partial last ones"""
    for w, h, sub in ((531, 45, 2), (523, 43, 1), (264, 40, 0), (520, 9, "L")):
        assert_gray(ctx, gray_file(w, h, sub, 75), d, (w, h, sub))


@pytest.mark.parametrize("orient", range(1, 9))
def test_gray_orientations(ctx, orient):
    """cv2 turns a grayscale read by the EXIF orientation as it turns a colour read"""
    from PIL import Image
    exif = Image.Exif()
    exif[0x0112] = orient
    for sub, (h, w) in ((2, (37, 53)), (1, (9, 300))):
        data = encode(synth_image(h, w, 3), quality=90, subsampling=sub, exif=exif)
        for d in G.SCALES:
            want = assert_gray(ctx, data, d, (orient, sub))
            assert want.shape == ((-(-w // d), -(-h // d)) if orient >= 5 else (-(-h // d), -(-w // d)))


@functools.lru_cache(maxsize=None)
def crafted_range_limit(sampling):
    """Y blocks that drive the inverse DCT into both ends of the range limit: flat blocks of sample value -100 .. 360 (DC only), blocks whose
    one horizontal, vertical or diagonal AC term swings +-160 and more around mid-grey, a block with only coefficient 63 set, and a block with
    all of them.  Chroma is noise.  Amplitudes stay within what an encoder can write for 8-bit samples (asserted)."""
    w, h = 16 * 8, 5 * 16
    (ybw, ybh), (cbw, cbh), _ = T.grids(w, h, sampling)
    rs = np.random.RandomState(12)
    y = np.zeros((ybw * ybh, 64), np.int64)
    flat = np.linspace(-100, 360, ybw * 2).round().astype(np.int64)
    y[:len(flat)] = T.dc_only(flat)
    at = len(flat)
    for pos in (1, 8, 9, 2, 16, 7, 56):
        for amp in (900, -900, 1000):
            y[at, pos] = amp
            y[at + 1, pos], y[at + 1, 0] = amp, 400
            y[at + 2, pos], y[at + 2, 0] = amp, -400
            at += 3
    for amp in (200, -200, 1000, -1000):
        y[at, 63] = amp                                                               # only the last zigzag position
        y[at + 1, 63], y[at + 1, 0], y[at + 1, 1] = amp, 300, -700
        at += 2
    assert at <= len(y)
    chroma = [rs.randint(-40, 41, (cbw * cbh, 64)) for _ in range(2)]
    f = T.craft(np.concatenate([y] + chroma), [T.ONES] * 3, w, h, sampling)
    T.assert_legitimate_amplitudes(f)
    return f


@pytest.mark.parametrize("sampling", ["4:4:4", "4:2:2", "4:2:0"])
def test_gray_range_limit_and_last_coefficient(ctx, sampling):
    f = crafted_range_limit(sampling)
    for d in G.SCALES:
        want = assert_gray(ctx, f.data, d, sampling)
        assert want.min() == 0 and want.max() == 255                                  # both ends were reached
    # coefficient 63 alone really shows at scale 1: a block that is not flat
    full = expected(f.data, 1)
    assert len(np.unique(full)) > 100


def test_gray_out_view_with_column_offset(ctx):
    """out= as a column-offset view of a wider tensor (odd offset: no store of the fast path is aligned): the image inside, nothing outside"""
    for sub, d, off in ((2, 1, 5), (1, 2, 3), (0, 4, 1), (2, 8, 7), (2, 1, 8)):
        data = gray_file(53, 37, sub, 95)
        want = expected(data, d)
        H, W = want.shape
        for dense in (False, True):
            wide = torch.full((H + 4, W + 24), 0xA5, dtype=torch.uint8, device=ctx.device)
            view = wide[2:2 + H, off:off + W]
            ret = ctx.imdecode(data, out=view, dense=dense, reduce=d, gray=True)
            assert ret.data_ptr() == view.data_ptr()
            host = wide.cpu().numpy()
            assert (host[2:2 + H, off:off + W] == want).all(), (sub, d, off, dense)
            host[2:2 + H, off:off + W] = 0xA5
            assert (host == 0xA5).all(), (sub, d, off, dense)
    with pytest.raises(ValueError, match="out must be"):
        ctx.imdecode(data, out=torch.empty((37, 53, 3), dtype=torch.uint8, device=ctx.device), gray=True)
    with pytest.raises(ValueError, match="dense"):
        ctx.imdecode(data, out=torch.empty((53, 37), dtype=torch.uint8, device=ctx.device).t(), gray=True)


def test_gray_batch_mixed_and_deterministic(ctx):
    """one imdecode_batch call over mixed sizes, samplings and gray-only files; the same batch twice gives identical bytes"""
    mixed = [gray_file(53, 37, 2, 95), gray_file(33, 17, "L", 30), gray_file(17, 17, 1, 95), gray_file(1, 1, 0, 30), gray_file(531, 45, 2, 75),
             gray_file(7, 5, "L", 95), restart_files()[2][1]]
    for d in G.SCALES:
        for dense in (False, True):
            first = ctx.imdecode_batch(mixed, threads=3, dense=dense, reduce=d, gray=True)
            again = ctx.imdecode_batch(mixed, threads=2, dense=dense, reduce=d, gray=True)
            assert isinstance(first, list) and len(first) == len(mixed)
            for data, a, b in zip(mixed, first, again):
                assert a.dim() == 2 and (a.cpu().numpy() == expected(data, d)).all(), (d, dense)
                assert a.shape == b.shape and bool((a == b).all())
    same = [gray_file(53, 37, sub, 95) for sub in (2, 1, 0, "L")]
    out = ctx.imdecode_batch(same, threads=4, reduce=2, gray=True)
    assert tuple(out.shape) == (4, 19, 27) and out.dtype == torch.uint8
    for data, t in zip(same, out):
        assert (t.cpu().numpy() == expected(data, 2)).all()
    # the colour read of the same context is untouched by the gray read before it
    import sv_oracle as o
    assert (ctx.imdecode(same[0]).cpu().numpy() == o.imdecode(same[0])).all()


@pytest.mark.parametrize("d", (1, 8))
def test_gray_photo(ctx, d):
    """sample_4.jpg, 2736 x 3648 at 4:2:0: the only large case"""
    want = G.pil_gray(photo(), d)
    got = ctx.imdecode(photo(), reduce=d, gray=True).cpu().numpy()
    assert got.shape == want.shape == (-(-3648 // d), -(-2736 // d)) and (got == want).all()


def test_imread_gray(ctx, golden_dir, tmp_path):
    from sudoku_vision_amd import imgcodecs as ic
    from sudoku_vision_amd._native import NativeError
    data = gray_file(53, 37, 2, 95)
    path = tmp_path / "cell.jpg"
    path.write_bytes(data)
    host = ic.imread(path, gray=True)
    assert isinstance(host, np.ndarray) and host.dtype == np.uint8 and (host == expected(data, 1)).all()
    dev = ic.imread(str(path), device=True, **ic.read_args_from_flags(ic.IMREAD_REDUCED_GRAYSCALE_2))
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and (dev.cpu().numpy() == expected(data, 2)).all()
    assert (ic.imdecode(np.frombuffer(data, np.uint8), gray=True, reduce=4) == expected(data, 4)).all()
    colour = ic.imread(path)
    assert colour.shape == (37, 53, 3)                                                # the colour read keeps its shape and meaning
    assert ic.imread(tmp_path / "missing.jpg", gray=True) is None
    assert ic.imdecode(data[:100], gray=True) is None and ic.imdecode(b"not a jpeg", gray=True) is None
    prog = tmp_path / "progressive.jpg"
    prog.write_bytes(encode(synth_image(32, 32, 1), quality=80, progressive=True))
    with pytest.raises(NativeError, match="progressive"):
        ic.imread(prog, gray=True)
    with pytest.raises(ValueError, match="reduce"):
        ic.imread(path, gray=True, reduce=3)
