"""Reduced-size JPEG decode (scale_denom 2, 4, 8), CPU part: the numpy restatement tests/jpeg_reduced_ref.py against Pillow's
libjpeg-turbo decode at the same scale, bit for bit, and the host-side argument checks of the scaled entries.

Pillow's reduced decode is Image.draft: it hands libjpeg the scale_denom cv2.IMREAD_REDUCED_COLOR_* hands it.  draft picks a smaller
reduction when a side is shorter than d, so pil_reduced_bgr() asserts the size it got: an unreduced decode cannot pass for a reduced
one.  Inputs compared with Pillow have both sides >= d; shapes below that are held against the size rule and a direct evaluation.
tests/test_gpu_jpeg_reduced.py decodes the same files on the GPU."""
import io
import os

import numpy as np
import pytest
from PIL import Image, ImageOps

import jpeg_reduced_ref as R
import sv_oracle as o
import test_jpeg_crafted as T
from test_jpeg import GOLDEN, encode, host, pil_bgr, synth_image  # noqa: F401  (host: fixture)

DENOMS = (2, 4, 8)
SHAPES = [(61, 83), (64, 80), (17, 9), (8, 8)]                                # (H, W)
SUBS = (0, 1, 2, "gray")
B_SIZES = [(9, 17), (17, 9), (33, 18), (34, 47)]                             # W x H of T.B_SIZES with both sides >= 8
# Every orientation x sampling x scale (full size too), which one colour kernel serves on the GPU (tests/test_gpu_jpeg_reduced.py runs
# these same cases).  (37, 51): partial MCUs; the reduced 4:2:2 chroma is wider than 2 at d = 2 and 4, so the h2v1 filter runs under
# the transposing orientations, and is replicated at d = 8.  (17, 9): chroma at most 2 wide, replication only.
ORIENT_SHAPES = [(37, 51), (17, 9)]                                           # (H, W)
SCALES = (1,) + DENOMS


def pil_reduced_bgr(data, d):
    """Pillow's decode at scale 1/d, EXIF orientation applied, RGB -> BGR"""
    im = Image.open(io.BytesIO(data))
    w, h = im.size
    assert w >= d and h >= d, "draft falls back to a smaller reduction below this"
    im.draft("L" if im.mode == "L" else "RGB", (max(1, w // d), max(1, h // d)))
    assert im.size == (R.ceil_div(w, d), R.ceil_div(h, d)), "Pillow did not reduce by d"
    return np.asarray(ImageOps.exif_transpose(im).convert("RGB"))[..., ::-1]


def synth_file(h, w, sub, orient=1, **kw):
    exif = Image.Exif()
    exif[0x0112] = orient
    extra = dict(exif=exif) if orient != 1 else {}
    if sub == "gray":
        return encode(synth_image(h, w, h * 131 + w, gray=True), quality=88, **extra, **kw)
    return encode(synth_image(h, w, h * 131 + w), quality=85, subsampling=sub, **extra, **kw)


def orientation_cases(d):
    """(what, data, expected BGR) at scale 1 / d: Pillow at the same scale; at d = 1 the full-size oracle"""
    for h, w in ORIENT_SHAPES:
        for sub in SUBS:
            for orient in range(1, 9):
                data = synth_file(h, w, sub, orient)
                yield (h, w, sub, orient), data, pil_reduced_bgr(data, d) if d > 1 else o.imdecode(data)


def crafted_files():
    """(name, data) of the crafted files of tests/test_jpeg_crafted.py the reduced kernels are held to: hard chroma, range-limit
    amplitudes, rank selection, block counts at component and workgroup boundaries"""
    out = [(f"b-{w}x{h}-{s}-{p}", T.file_b(w, h, s, p).data) for w, h in B_SIZES for s in ("4:2:0", "4:2:2") for p in T.B_PATTERNS]
    out += [(f"c-{s}-{ri}", T.file_c(s, ri).data) for s in ("gray", "4:2:0") for ri in (0, 2)]
    out += [(f"e-{s}-{w}x{h}", T.file_e(s, w, h).data) for s, w, h in T.E_CASES]
    out += [("a-yramp", T.file_a("yramp").data)]
    return out


def assert_equal(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert (got == want).all(), (what, int((got != want).sum()))


@pytest.mark.parametrize("d", DENOMS)
@pytest.mark.parametrize("sub", SUBS)
def test_restatement_matches_pillow_synthetic(sub, d):
    for h, w in SHAPES:
        data = synth_file(h, w, sub)
        assert_equal(R.decode_file(data, d), pil_reduced_bgr(data, d), (h, w))


@pytest.mark.parametrize("d", DENOMS)
def test_restatement_matches_pillow_crafted(d):
    for name, data in crafted_files():
        assert_equal(R.decode_file(data, d), pil_reduced_bgr(data, d), name)


@pytest.mark.parametrize("d", DENOMS)
def test_restatement_range_limit(d):
    """T.file_d: one flat block per sample value 128 + k.  As at full size (tests/test_jpeg_crafted.py::test_d_range_limit) libjpeg's table
    wraps to 0 from k = 512 on where libjpeg-turbo's SIMD code may saturate, so Pillow is the judge up to k = 511; a flat block of value v
    stays flat at every scale, which is asserted for those k directly."""
    f = T.file_d()
    ks = np.array(T.d_offsets())
    S = 8 // d
    got, pil = R.decode_file(f.data, d), pil_reduced_bgr(f.data, d)
    assert got.shape == pil.shape == (S, S * len(ks), 3)
    same = (got == pil).reshape(S, len(ks), S, 3).all(axis=(0, 2, 3))
    print(f"d={d}: restatement == Pillow for k in", ks[same].tolist(), "and differs for k in", ks[~same].tolist())
    assert same[ks <= 511].all()
    want = np.where(ks < -128, 0, np.where(ks > 127, 255, 128 + ks))[ks <= 511]
    assert (got.reshape(S, len(ks), S, 3)[:, ks <= 511] == want[None, :, None, None]).all()


@pytest.mark.parametrize("d", DENOMS)
def test_restatement_matches_pillow_photo(d):
    data = open(os.path.join(GOLDEN, "sample_1.jpg"), "rb").read()
    want = pil_reduced_bgr(data, d)
    assert want.shape == (R.ceil_div(3648, d), R.ceil_div(2736, d), 3)
    assert_equal(R.decode_file(data, d), want)


@pytest.mark.parametrize("orient", range(1, 9))
def test_restatement_orientations(orient):
    for d in DENOMS:
        data = synth_file(61, 83, 2, orient)
        want = pil_reduced_bgr(data, d)
        ow, oh = R.scaled_size(83, 61, d)
        assert want.shape == ((ow, oh, 3) if orient >= 5 else (oh, ow, 3))
        assert_equal(R.decode_file(data, d), want, d)


@pytest.mark.parametrize("d", SCALES)
def test_restatement_orientations_samplings_scales(d):
    """the expected images the GPU test uses, before a GPU sees them: Pillow's against the restatement; at d = 1 the oracle's against
    Pillow's full-size decode (the restatement has no h2v2 up-sampling: 4:2:0 at full size is not a reduced decode)"""
    for what, data, want in orientation_cases(d):
        ow, oh = R.scaled_size(what[1], what[0], d)
        assert want.shape == ((ow, oh, 3) if what[3] >= 5 else (oh, ow, 3)), what
        assert_equal(R.decode_file(data, d) if d > 1 else pil_bgr(data), want, what)


def test_scale_one_is_the_full_decode():
    """d = 1 of the restatement is the decode the front end already has: 8x8 blocks, h2v1 where 4:2:2 needs it"""
    for sub in (0, 1, "gray"):
        data = synth_file(61, 83, sub)
        assert_equal(R.decode_file(data, 1), o.imdecode(data), sub)


def test_block_sizes():
    assert R.block_sizes(2, 3, 2, 2) == [4, 8, 8] and R.block_sizes(4, 3, 2, 2) == [2, 4, 4] and R.block_sizes(8, 3, 2, 2) == [1, 2, 2]
    for d in DENOMS:
        assert R.block_sizes(d, 3, 2, 1) == [8 // d] * 3 and R.block_sizes(d, 3, 1, 1) == [8 // d] * 3 and R.block_sizes(d, 1, 1, 1) == [8 // d]


@pytest.mark.parametrize("sampling", ["gray", "4:4:4", "4:2:2", "4:2:0"])
@pytest.mark.parametrize("w,h", [(7, 3), (3, 4), (1, 1), (5, 9)])
def test_sides_below_d(sampling, w, h):
    """Pillow's draft does not reduce these by d, so they are held to the size rule and to a direct evaluation: a DC-only file whose
    blocks are flat (DC = 8 x (value - 128), quantiser 1: every reduced transform returns the value exactly)."""
    ncomp = T.SAMPLINGS[sampling][0]
    n = sum(bw * bh for bw, bh in T.grids(w, h, sampling))
    flat = [200, 90, 170][:ncomp]
    vals = np.concatenate([np.full(bw * bh, v) for v, (bw, bh) in zip(flat, T.grids(w, h, sampling))])
    assert len(vals) == n
    f = T.craft(T.dc_only(vals), [T.ONES] * ncomp, w, h, sampling)
    px = R.ycc_to_bgr(*[np.array(v) for v in flat])[None, None] if ncomp == 3 else np.full((1, 1, 3), flat[0], np.uint8)
    for d in DENOMS:
        got = R.decode_file(f.data, d)
        assert got.shape == (R.ceil_div(h, d), R.ceil_div(w, d), 3)
        assert (got == px).all(), d
    assert (o.imdecode(f.data) == px).all()


# ---- host-side argument checks of the scaled entries (no GPU needed) ----
def test_scaled_size_entry(host):
    import ctypes as C
    from sudoku_vision_amd import _native
    lib = _native.lib()
    for h, w in [(61, 83), (17, 9), (8, 8), (1, 1), (3648, 2736), (7, 3)]:
        for orient in (1, 6):
            info = host.jpeg_parse(synth_file(h, w, 2, orient))
            assert (info.out_width, info.out_height) == ((h, w) if orient == 6 else (w, h))
            for d in R.SCALES:
                ow, oh = C.c_int(-1), C.c_int(-1)
                assert lib.sv_jpeg_scaled_size(C.byref(info), d, C.byref(ow), C.byref(oh)) == 0
                sw, sh = R.scaled_size(w, h, d)
                assert (ow.value, oh.value) == ((sh, sw) if orient == 6 else (sw, sh)), (h, w, orient, d)
    for bad in (0, 3, 5, 16, -2):
        assert lib.sv_jpeg_scaled_size(C.byref(info), bad, C.byref(ow), C.byref(oh)) == -1
        assert b"scale_denom" in lib.sv_last_error()
    assert lib.sv_jpeg_scaled_size(None, 2, C.byref(ow), C.byref(oh)) == -1


def test_bad_scale_denom_is_bad_arg(host):
    """the reconstruct entries refuse a scale_denom outside {1, 2, 4, 8} before they look at anything else"""
    import ctypes as C
    from sudoku_vision_amd import _native
    lib = _native.lib()
    info = host.jpeg_parse(synth_file(16, 16, 2))
    for bad in (0, 3, 16, -1):
        assert lib.sv_jpeg_reconstruct_scaled_bgr_u8(None, C.byref(info), None, None, None, 0, None, bad) == -1
        assert b"scale_denom" in lib.sv_last_error()
        assert lib.sv_jpeg_reconstruct_sparse_scaled_bgr_u8(None, C.byref(info), None, None, None, None, None, 0, None, bad) == -1
        assert b"scale_denom" in lib.sv_last_error()


def test_imread_reduced_flags():
    """cv2's flag values, and their mapping to reduce=; a bad reduce is a ValueError before any GPU work"""
    from sudoku_vision_amd import imgcodecs
    assert (imgcodecs.IMREAD_COLOR, imgcodecs.IMREAD_REDUCED_COLOR_2, imgcodecs.IMREAD_REDUCED_COLOR_4, imgcodecs.IMREAD_REDUCED_COLOR_8) == (1, 17, 33, 65)
    assert [imgcodecs.reduce_from_flags(f) for f in (1, 17, 33, 65)] == [1, 2, 4, 8]
    for flags in (0, 16, 32, 64, 2, -1):                                      # grayscale and anydepth reads are not this front end's
        with pytest.raises(ValueError):
            imgcodecs.reduce_from_flags(flags)
    for bad in (0, 3, 16, "2"):
        with pytest.raises(ValueError, match="reduce"):
            imgcodecs.imdecode(b"", reduce=bad)
        with pytest.raises(ValueError, match="reduce"):
            imgcodecs.imread(os.path.join(GOLDEN, "sample_1.jpg"), reduce=bad)
