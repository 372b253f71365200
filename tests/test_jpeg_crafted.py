"""The JPEG front end on files whose coefficients the tests choose (tests/jpeg_craft.py), not Pillow's encoder: CPU part.

Every crafted file is opened by Pillow; the oracle (oracle/sv_jpeg_oracle.c) decodes it to Pillow's pixels; the product's host entropy
decoder (csrc/host_jpeg.cpp), dense and compact, returns exactly the coefficients that were written.  tests/test_gpu_jpeg_crafted.py
decodes the same files on the GPU.  The files, by what they are hard for:

  (a) colour conversion: every (Cb, Cr) pair under Y = 0, Y = 255 and a varying Y, as flat 8x8 blocks of a 2048x2048 4:4:4 file
  (b) chroma up-sampling: 4:2:0 / 4:2:2 chroma that alternates 0/255 per sample, at the chroma sizes where the filter changes form
  (c) the compact transport's rank selection: full blocks, empty blocks, blocks with only the last zigzag positions
  (d) range_limit: one flat block per sample value around every breakpoint of libjpeg's table
  (e) block counts of 31, 32, 33 and component boundaries inside a 32-block workgroup
  (f) the eight orientations on frames more than one 256-pixel workgroup wide

Stated limit: the kernel's idct8 works in 32-bit int, libjpeg's C code in long, libjpeg-turbo's SIMD code on 16-bit intermediates.  They
agree while the dequantised coefficients and the first pass's outputs fit 16 bits, which every file here asserts or has by construction
(DC-only blocks); nothing here feeds values beyond that.
"""
import functools
import io
from collections import namedtuple

import numpy as np
import pytest
from PIL import Image

import sv_oracle as o
from jpeg_craft import _ZZ, SAMPLINGS, STD_HUFFMAN, write_jpeg
from test_jpeg import _densify, _parse_tables, encode, host, pil_bgr, synth_image  # noqa: F401  (host: fixture)

Crafted = namedtuple("Crafted", "data coef quant width height sampling orientation")
ONES = np.ones(64, np.int64)


def craft(coef, quant, width, height, sampling, **kw):
    coef = np.ascontiguousarray(coef, np.int16).ravel()
    quant = np.asarray(quant, np.int64).reshape(-1, 64)
    return Crafted(write_jpeg(coef, quant, width, height, sampling, **kw), coef, quant, width, height, sampling, kw.get("orientation", 1))


def grids(width, height, sampling):
    """[(blocks across, blocks down)] of each component's padded block grid"""
    ncomp, hs, vs = SAMPLINGS[sampling]
    mcux, mcuy = -(-width // (8 * hs)), -(-height // (8 * vs))
    return [(mcux * hs, mcuy * vs)] + [(mcux, mcuy)] * (ncomp - 1)


def dc_only(values):
    """sample values (any shape) -> DC-only blocks that decode, with quantisers of 1, to flat blocks of exactly those values: the DC term
    of the 8x8 DCT is 8 x the mean, and both passes of the integer inverse DCT are exact on a multiple of 8"""
    blocks = np.zeros((np.size(values), 64), np.int64)
    blocks[:, 0] = 8 * (np.asarray(values, np.int64).ravel() - 128)
    return blocks


# ---- the 8x8 DCT in float64, and pass 1 of libjpeg's integer inverse (jidctint.c, CONST_BITS 13, PASS1_BITS 2) ----
_C = np.array([[(np.sqrt(0.5) if u == 0 else 1.0) / 2 * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])


def fdct_plane(plane):
    """u8-range plane [8*bh, 8*bw] -> rounded coefficients of (plane - 128), [bh*bw, 64] natural order"""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    f = (plane.astype(np.float64) - 128).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
    return np.rint(_C @ f @ _C.T).astype(np.int64).reshape(bh * bw, 64)


def idct_float(deq):
    """dequantised blocks [n, 64] -> samples [n, 8, 8] before rounding and clamping"""
    return _C.T @ deq.reshape(-1, 8, 8).astype(np.float64) @ _C + 128


def idct_pass1(deq):
    """the integer column pass on dequantised blocks [n, 64] -> workspace [n, 8, 8], in int64 (no wrap-around to hide an overflow)"""
    d = deq.reshape(-1, 8, 8).astype(np.int64)
    i0, i1, i2, i3, i4, i5, i6, i7 = (d[:, k, :] for k in range(8))
    z1 = (i2 + i6) * 4433
    t2, t3 = z1 - i6 * 15137, z1 + i2 * 6270
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    z1, z2, z3, z4 = i7 + i1, i5 + i3, i7 + i3, i5 + i1
    z5 = (z3 + z4) * 9633
    z3, z4 = z5 - z3 * 16069, z5 - z4 * 3196
    z1, z2 = -z1 * 7373, -z2 * 20995
    o0, o1, o2, o3 = i7 * 2446 + z1 + z3, i5 * 16819 + z2 + z4, i3 * 25172 + z2 + z3, i1 * 12299 + z1 + z4
    rows = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
    return (np.stack(rows, 1) + (1 << 10)) >> 11


def assert_legitimate_amplitudes(f):
    """the stated limit: dequantised coefficients and pass-1 outputs fit 16 bits"""
    ncomp = SAMPLINGS[f.sampling][0]
    q = np.concatenate([np.broadcast_to(f.quant[c], (bw * bh, 64)) for c, (bw, bh) in zip(range(ncomp), grids(f.width, f.height, f.sampling))])
    deq = f.coef.astype(np.int64).reshape(-1, 64) * q
    assert np.abs(deq).max() <= 32767
    ws = idct_pass1(deq)
    assert ws.min() >= -32768 and ws.max() <= 32767
    return deq


# ---- (a) colour conversion, exhaustive in (Cb, Cr) ----
A_LUMA = ("y0", "y255", "yramp")


def a_planes(luma):
    """sample value of block (i, j) of each component: Cb = i, Cr = j"""
    i, j = np.mgrid[0:256, 0:256]
    y = {"y0": np.zeros_like(i), "y255": np.full_like(i, 255), "yramp": (7 * i + 13 * j) % 256}[luma]
    return y, i, j


@functools.lru_cache(maxsize=None)
def file_a(luma):
    return craft(np.concatenate([dc_only(p) for p in a_planes(luma)]), [ONES] * 3, 2048, 2048, "4:4:4")


# ---- (b) chroma up-sampling on chroma that alternates per sample ----
B_SIZES = [(5, 1), (6, 3), (7, 5), (9, 17), (10, 6), (33, 18), (34, 47),      # W x H; chroma widths 3, 3, 4, 5, 5, 17, 17
           (15, 4), (16, 2), (17, 9), (18, 4)]                                 # chroma widths 8, 8, 9, 9
B_PATTERNS = ("alt_x", "alt_y", "checker", "random")
B_CASES = [(w, h, s, p) for w, h in B_SIZES for s in ("4:2:0", "4:2:2") for p in B_PATTERNS]


@functools.lru_cache(maxsize=None)
def file_b(w, h, sampling, pattern):
    (ybw, ybh), (cbw, cbh), _ = grids(w, h, sampling)
    yy, xx = np.mgrid[0:8 * cbh, 0:8 * cbw]
    rs = np.random.RandomState(1000 * w + 10 * h + B_PATTERNS.index(pattern))
    chroma = []
    for c in range(2):                                                        # Cr is Cb's pattern one sample out of phase
        t = {"alt_x": (xx + c) % 2, "alt_y": (yy + c) % 2, "checker": (xx + yy + c) % 2, "random": rs.randint(0, 2, xx.shape)}[pattern]
        chroma.append(fdct_plane(255 * t))
    return craft(np.concatenate([np.zeros((ybw * ybh, 64), np.int64)] + chroma), [ONES] * 3, w, h, sampling)


# ---- (c) rank selection in the compact transport ----
C_KINDS = ("full", "zero", "zz63", "dc", "zz62_63", "low", "high")
C_POSITIONS = {"full": range(64), "zero": (), "zz63": (63,), "dc": (0,), "zz62_63": (62, 63), "low": range(32), "high": range(32, 64)}


def c_kinds(n):
    """kind of each of a component's n blocks: the cycle; first and last block full; and full, zero, full before the end, so that an empty
    block (mask 0, its offset the next block's) lies between two blocks that use all 64 ranks"""
    kinds = [C_KINDS[i % 7] for i in range(n)]
    kinds[-4:] = ["full", "zero", "full", "full"]
    return kinds


@functools.lru_cache(maxsize=None)
def file_c(sampling, restart_interval=0):
    rs = np.random.RandomState(63 + len(sampling))
    comps = grids(48, 40, sampling)
    blocks = []
    for bw, bh in comps:
        for kind in c_kinds(bw * bh):
            zz = np.zeros(64, np.int64)
            for z in C_POSITIONS[kind]:
                zz[z] = rs.choice([-2, -1, 1, 2])
            if kind == "dc":
                zz[0] = rs.choice([-40, -23, 17, 40])
            blk = np.zeros(64, np.int64)
            blk[_ZZ] = zz
            blocks.append(blk)
    quant = rs.randint(1, 4, (len(comps), 64))                               # 1..3: 64 coefficients of +-2 stay within +-96 of mid-grey
    return craft(np.stack(blocks), quant, 48, 40, sampling, restart_interval=restart_interval)


# ---- (d) range_limit ----
def d_offsets():
    """k of each block (sample value 128 + k).  The first block, k = -200, is only a step on the way down: the first DC difference the
    standard tables can code is 11 bits, and k = -400 needs a DC of -3200."""
    ks = set(range(-400, 521, 16)) | {520}
    for b in (-384, -128, 0, 128, 384):
        ks |= {b - 1, b, b + 1}
    return [-200] + sorted(ks)


@functools.lru_cache(maxsize=None)
def file_d():
    ks = d_offsets()
    return craft(dc_only(128 + np.array(ks)), [ONES], 8 * len(ks), 8, "gray")


@functools.lru_cache(maxsize=None)
def d_agreement():
    """per block of file_d: does the oracle's decode equal Pillow's?"""
    f = file_d()
    same = o.imdecode(f.data) == pil_bgr(f.data)
    return same.reshape(8, -1, 8, 3).all(axis=(0, 2, 3))


# ---- (e) workgroup and component boundaries ----
E_CASES = [("gray", 8, 248), ("gray", 8, 256), ("gray", 8, 264),             # 31, 32, 33 blocks
           ("4:2:0", 80, 16),                                                 # 20 + 5 + 5: both boundaries inside workgroup 0
           ("4:2:0", 112, 32),                                                # 56 + 14 + 14: Y/Cb inside workgroup 1
           ("4:2:2", 72, 8), ("4:4:4", 72, 8)]


@functools.lru_cache(maxsize=None)
def file_e(sampling, w, h, orientation=1):
    n = sum(bw * bh for bw, bh in grids(w, h, sampling))
    values = (37 * np.arange(n) + 11) % 256                                   # distinct: 37 is odd and n <= 256
    assert n <= 256 and len(set(values)) == n
    return craft(dc_only(values), [ONES] * SAMPLINGS[sampling][0], w, h, sampling, orientation=orientation)


# ---- (f) orientations on frames wider than one workgroup ----
F_SHAPES = [(9, 300), (300, 9), (263, 521), (257, 256)]                      # (H, W)
F_CASES = [(h, w, orient, sub) for h, w in F_SHAPES for orient in range(1, 9) for sub in (0, 1, 2)]
F_CRAFTED = [(s, w, h, orient) for s, w, h in E_CASES if s == "4:2:0" for orient in (5, 6, 7, 8)]


@functools.lru_cache(maxsize=None)
def file_f(h, w, orient, sub):
    exif = Image.Exif()
    exif[0x0112] = orient
    return encode(synth_image(h, w, h + w + orient), quality=90, subsampling=sub, exif=exif)


# ---- the checks every crafted file gets ----
def densify(info, masks, offs, vals):
    """test_jpeg._densify without the Python loop over blocks, for the 196,608-block files of (a)"""
    bits = ((masks[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)       # [blocks, zigzag position]
    rank = np.cumsum(bits, 1) - 1
    out = np.zeros((len(masks), 64), np.int16)
    b, z = np.nonzero(bits)
    out[b, np.array(_ZZ)[z]] = vals[offs[b].astype(np.int64) + rank[b, z]]
    return out.ravel()


def check_file(host, f, pixels=True):
    im = Image.open(io.BytesIO(f.data))
    assert im.size == (f.width, f.height) and im.mode == ("L" if f.sampling == "gray" else "RGB")
    want = pil_bgr(f.data)
    assert want.shape == ((f.width, f.height, 3) if f.orientation >= 5 else (f.height, f.width, 3))
    if pixels:
        assert (o.imdecode(f.data) == want).all()
    ncomp = SAMPLINGS[f.sampling][0]
    oc, oq = o.jpeg_coefficients(f.data)
    assert (oc == f.coef).all() and (oq == f.quant).all()
    info, coef, quant = host.jpeg_entropy_decode(f.data)
    assert info.coef_count == f.coef.size and info.orientation == f.orientation
    assert (coef == f.coef).all() and (quant[:ncomp] == f.quant).all()
    info2, masks, offs, vals, quant2 = host.jpeg_entropy_decode_sparse(f.data)
    assert len(vals) <= info2.sparse_capacity <= info2.coef_count and (quant2[:ncomp] == f.quant).all()
    assert int(sum(bin(int(m)).count("1") for m in masks[:4096])) == np.count_nonzero(f.coef[:64 * 4096])
    dense = densify if len(masks) > 4096 else _densify
    assert (dense(info2, masks, offs, vals) == f.coef).all()
    return want


# ---- the writer itself ----
def test_standard_tables_are_pillows():
    """the Annex K tables written out in jpeg_craft.py are what libjpeg puts into a file with optimize=False"""
    dht = _parse_tables(encode(synth_image(16, 16, 1), quality=80, subsampling=2))[1]
    assert dht == STD_HUFFMAN


def test_writer_refuses_what_the_standard_tables_cannot_code():
    blk = np.zeros((1, 64), np.int16)
    for pos, ok, bad in ((0, 2047, 2048), (0, -2047, -2048), (1, 1023, 1024), (63, -1023, -1024)):
        blk[:] = 0
        blk[0, pos] = ok
        data = write_jpeg(blk, [ONES], 8, 8, "gray")
        assert (o.jpeg_coefficients(data)[0] == blk.ravel()).all()
        blk[0, pos] = bad
        with pytest.raises(ValueError, match="bits"):
            write_jpeg(blk, [ONES], 8, 8, "gray")
    two = np.zeros((2, 64), np.int16)
    two[:, 0] = (1024, -1024)                                                # each codable on its own, their difference is not
    with pytest.raises(ValueError, match="DC difference"):
        write_jpeg(two, [ONES], 16, 8, "gray")
    with pytest.raises(ValueError):
        write_jpeg(blk[:, :63], [ONES], 8, 8, "gray")
    with pytest.raises(ValueError):
        write_jpeg(np.zeros((1, 64), np.int16), [ONES * 256], 8, 8, "gray")
    with pytest.raises(ValueError):
        write_jpeg(np.zeros((1, 64), np.int16), [ONES], 8, 8, "4:1:1")


@pytest.mark.parametrize("sampling", ["gray", "4:2:0"])
@pytest.mark.parametrize("interval", [1, 2, 5])
def test_writer_restart_intervals(host, sampling, interval):
    """DRI + RSTn: same coefficients, same pixels as the file without them; decoded on several threads too"""
    f, plain = file_c(sampling, interval), file_c(sampling)
    assert f.data.count(b"\xff\xdd") == 1 and o.jpeg_info(f.data).restart_interval == interval
    assert (check_file(host, f) == pil_bgr(plain.data)).all()
    assert (host.jpeg_entropy_decode(f.data, threads=3)[1] == f.coef).all()


# ---- (a) ----
@pytest.mark.parametrize("luma", A_LUMA)
def test_a_colour_conversion_exhaustive(host, luma):
    f = file_a(luma)
    check_file(host, f)
    im = Image.open(io.BytesIO(f.data))
    im.draft("YCbCr", im.size)                                               # libjpeg's planes before its colour conversion
    assert im.mode == "YCbCr"
    got = np.asarray(im)
    for c, plane in enumerate(a_planes(luma)):                               # every block decodes to a flat block of exactly its value
        assert (got[..., c].reshape(256, 8, 256, 8) == plane[:, None, :, None]).all()


# ---- (b) ----
@pytest.mark.parametrize("w,h,sampling,pattern", B_CASES)
def test_b_chroma_upsampling_hard_chroma(host, w, h, sampling, pattern):
    f = file_b(w, h, sampling, pattern)
    assert_legitimate_amplitudes(f)
    check_file(host, f)


def test_b_chroma_really_alternates():
    """the rounded coefficients still decode to chroma that swings over (nearly) the whole range between neighbouring samples"""
    f = file_b(34, 47, "4:2:0", "checker")
    n_y = grids(34, 47, "4:2:0")[0]
    cb = idct_float(f.coef.reshape(-1, 64)[n_y[0] * n_y[1]:].astype(np.int64))
    assert cb.min() < 8 and cb.max() > 247 and np.abs(np.diff(cb, axis=2)).min() > 200


# ---- (c) ----
@pytest.mark.parametrize("sampling", ["gray", "4:2:0"])
def test_c_sparse_rank_selection(host, sampling):
    f = file_c(sampling)
    samples = idct_float(assert_legitimate_amplitudes(f))
    assert samples.min() >= 1 and samples.max() <= 254                       # no clamp hides a wrong coefficient (the integer IDCT is within 1 of this)
    check_file(host, f)
    _, masks, offs, vals, _ = host.jpeg_entropy_decode_sparse(f.data)
    full, off = np.uint64(0xFFFFFFFFFFFFFFFF), 0
    assert {int(x) for x in masks} >= {1 << 63, 1, 3 << 62, (1 << 32) - 1, ((1 << 32) - 1) << 32}
    for (bw, bh) in grids(48, 40, sampling):                                 # the transport holds the cases the file was built for
        m = masks[off:off + bw * bh]
        assert m[0] == full and m[-1] == full and (m[-4], m[-3], m[-2]) == (full, 0, full)
        off += bw * bh
    if sampling == "gray":                                                   # scan order = storage order: the empty block repeats the next block's offset
        assert offs[-3] == offs[-2] == offs[-4] + 64


def test_densify_vectorised_equals_loop(host):
    info, masks, offs, vals, _ = host.jpeg_entropy_decode_sparse(file_c("4:2:0").data)
    assert (densify(info, masks, offs, vals) == _densify(info, masks, offs, vals)).all()


# ---- (d) ----
def test_d_range_limit(host):
    """One flat block per sample value 128 + k, k from -400 to 520.  libjpeg's C code looks the value up in a table indexed (x & 1023),
    which wraps to 0 from k = 512 on; libjpeg-turbo's SIMD inverse DCT saturates to 255 there instead.  Up to k = 511 the two describe
    the same function, so there the oracle must equal Pillow; beyond it the agreement is measured, not asserted.
    Measured with libjpeg-turbo's SIMD code: oracle == Pillow for every k of the file from -400 to 496 (sample values clamp to 0 up to
    k = -128 and to 255 from k = 127); they differ at k = 512 and 520 (oracle 0, Pillow 255)."""
    f = file_d()
    check_file(host, f, pixels=False)
    ks = np.array(d_offsets())
    agree = d_agreement()
    print("range_limit: oracle == Pillow for k in", ks[agree].tolist(), "and differs for k in", ks[~agree].tolist())
    assert agree[ks <= 511].all()
    img = o.imdecode(f.data)
    want = np.where(ks < -128, 0, np.where(ks > 127, 255, 128 + ks))[ks <= 511]
    assert (img.reshape(8, -1, 8, 3)[:, ks <= 511] == want[None, :, None, None]).all()


# ---- (e) ----
@pytest.mark.parametrize("sampling,w,h", E_CASES)
def test_e_block_counts_and_component_boundaries(host, sampling, w, h):
    f = file_e(sampling, w, h)
    want = check_file(host, f)
    if sampling == "gray":                                                   # each block is its own flat value
        assert (want[::8, ::8, 0].ravel() == (37 * np.arange(w * h // 64) + 11) % 256).all()


# ---- (f) ----
@pytest.mark.parametrize("h,w", F_SHAPES)
def test_f_orientations_wide_oracle(h, w):
    for orient in range(1, 9):
        for sub in (0, 1, 2):
            data = file_f(h, w, orient, sub)
            want = pil_bgr(data)
            assert want.shape == ((w, h, 3) if orient >= 5 else (h, w, 3))
            assert (o.imdecode(data) == want).all(), (orient, sub)


@pytest.mark.parametrize("sampling,w,h,orient", F_CRAFTED)
def test_f_orientations_crafted(host, sampling, w, h, orient):
    f = file_e(sampling, w, h, orient)
    want = check_file(host, f)
    if orient == 5:                                                          # the plain transpose
        assert (want == pil_bgr(file_e(sampling, w, h).data).transpose(1, 0, 2)).all()
