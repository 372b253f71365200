"""CPU: the PNG encoder's host half through the C ABI (csrc/host_png.cpp: sv_png_encode_plan, sv_png_assemble, _batch).  The bands are made here with
raw zlib streams (wbits -15, Z_RLE, ended by Z_SYNC_FLUSH: a whole number of bytes, no final block) of the restatement's filtered bytes and their
Adler-32; the assembled file must have chunk CRCs that verify, an IDAT that zlib.decompress accepts (that checks the combined Adler-32), and
Pillow must decode it to exactly the input."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import png_encode_ref as R

BAD_ARG, UNSUPPORTED, BUFFER = -1, -4, -6


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    import sudoku_vision_amd as sva
    if not os.path.exists(sva._native.LIB_PATH):
        g.build()
    return sva._native.lib()


def make_plan(lib, W, H, ch, band_rows, filter=1, strategy=0):
    from sudoku_vision_amd._native import PngEnc
    plan = PngEnc()
    rc = lib.sv_png_encode_plan(W, H, ch, filter, strategy, band_rows, C.byref(plan))
    assert rc == 0, lib.sv_last_error()
    return plan


def zlib_bands(img, plan, mode="sub"):
    """(stream bytes, band_len u32, adler u32): every band a raw deflate stream of its own"""
    f = R.filtered(img, mode)
    per = plan.band_rows * plan.row_bytes
    parts, adlers = [], []
    for b in range(plan.bands):
        piece = f[b * per:(b + 1) * per]
        c = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
        parts.append(c.compress(piece) + c.flush(zlib.Z_SYNC_FLUSH))
        adlers.append(zlib.adler32(piece))
    return b"".join(parts), np.array([len(p) for p in parts], np.uint32), np.array(adlers, np.uint32)


def assemble(lib, plan, stream, lens, adlers, cap=None):
    buf = np.frombuffer(stream + b"\0", np.uint8)                       # never an empty buffer
    cap = int(plan.out_bound) if cap is None else cap
    out = np.zeros(max(cap, 1), np.uint8)
    size = C.c_size_t()
    rc = lib.sv_png_assemble(C.byref(plan), buf.ctypes.data, lens.ctypes.data, adlers.ctypes.data, out.ctypes.data, cap, C.byref(size))
    return rc, out[:size.value].tobytes() if rc == 0 else size.value


@pytest.mark.parametrize("bands", [1, 2, 7])
def test_assembled_file_decodes(lib, bands):
    for gray in (False, True):
        for kind in ("synthetic", "noise", "zeros"):
            H, W = 21, 30
            img = R.content(kind, H, W, gray)
            plan = make_plan(lib, W, H, 1 if gray else 3, -(-H // bands))
            assert plan.bands == bands and plan.row_bytes == 1 + W * (1 if gray else 3) and plan.filtered_bytes == H * plan.row_bytes
            assert plan.stream_bound == plan.filtered_bytes + 10 * bands and plan.out_bound >= plan.stream_bound + 65
            stream, lens, adlers = zlib_bands(img, plan)
            assert (lens <= plan.band_rows * plan.row_bytes + 10).all()     # what zlib writes for a band fits the bound this encoder states
            rc, data = assemble(lib, plan, stream, lens, adlers)
            assert rc == 0, lib.sv_last_error()
            assert len(data) == len(stream) + 65
            assert R.check_file(data, img) == R.filtered(img, "sub")
            got, mode, size = R.pillow_decode(data)
            assert mode == ("L" if gray else "RGB") and size == (W, H) and (got == img).all()
            # the IDAT is exactly: header, bands, final empty block, Adler-32 of all filtered bytes
            idat = R.parse(data)[1][1]
            assert idat == b"\x78\x01" + stream + b"\x03\x00" + zlib.adler32(R.filtered(img, "sub")).to_bytes(4, "big")


def test_band_of_no_bytes_plus_the_empty_block(lib):
    """A band may contribute nothing but its closing empty stored block (0 + 5 bytes): here the first band's stream carries the filtered bytes of
    both bands and the second band's is 00 00 00 ff ff.  The host half only concatenates; the per-band Adler sums still combine by the bands' own
    byte counts.  At the other end a band of stored blocks is its bytes + 5 + 5: exactly the bound."""
    img = R.content("zeros", 8, 9, gray=True)
    img[3, 4] = 200
    plan = make_plan(lib, 9, 8, 1, 4)
    f = R.filtered(img, "sub")
    c = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
    both = c.compress(f) + c.flush(zlib.Z_SYNC_FLUSH)
    empty = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_RLE).flush(zlib.Z_SYNC_FLUSH)
    assert empty == b"\x00\x00\x00\xff\xff" and len(both) <= 40 + 10
    adlers = np.array([zlib.adler32(f[:40]), zlib.adler32(f[40:])], np.uint32)
    rc, data = assemble(lib, plan, both + empty, np.array([len(both), 5], np.uint32), adlers)
    assert rc == 0 and R.check_file(data, img) == f and (R.pillow_decode(data)[0] == img).all()
    # stored bands: level 0 writes 5 + bytes, the sync flush 5 more
    img = R.content("noise", 8, 9, gray=True)
    f = R.filtered(img, "sub")
    parts = []
    for k in range(2):
        c = zlib.compressobj(0, zlib.DEFLATED, -15)
        parts.append(c.compress(f[40 * k:40 * k + 40]) + c.flush(zlib.Z_SYNC_FLUSH))
    assert [len(p) for p in parts] == [50, 50]
    adlers = np.array([zlib.adler32(f[:40]), zlib.adler32(f[40:])], np.uint32)
    rc, data = assemble(lib, plan, b"".join(parts), np.array([50, 50], np.uint32), adlers)
    assert rc == 0 and len(data) == 100 + 65 and R.check_file(data, img) == f and (R.pillow_decode(data)[0] == img).all()


def test_batch_and_threads(lib):
    H, W = 16, 20
    imgs = [R.content(kind, H, W) for kind in ("synthetic", "noise", "zeros", "flat")]
    plan = make_plan(lib, W, H, 3, 5)
    bands = [zlib_bands(i, plan) for i in imgs]
    singles = [assemble(lib, plan, *b)[1] for b in bands]
    for i, s in zip(imgs, singles):
        assert (R.pillow_decode(s)[0] == i).all()
    n = len(imgs)
    for threads in (1, 3, 16):
        streams = [np.frombuffer(b[0] + b"\0", np.uint8) for b in bands]
        outs = [np.zeros(int(plan.out_bound), np.uint8) for _ in range(n)]
        VP = C.c_void_p * n
        sizes, status = (C.c_size_t * n)(), (C.c_int * n)()
        rc = lib.sv_png_assemble_batch(C.byref(plan), n, VP(*[s.ctypes.data for s in streams]), VP(*[b[1].ctypes.data for b in bands]), VP(*[b[2].ctypes.data for b in bands]),
                                       VP(*[o.ctypes.data for o in outs]), (C.c_size_t * n)(*[o.size for o in outs]), sizes, threads, status)
        assert rc == 0 and list(status) == [0] * n
        assert [outs[i][:sizes[i]].tobytes() for i in range(n)] == singles
    # one short buffer: its status says so, the others are written
    caps = [o.size for o in outs]
    caps[2] = len(singles[2]) - 1
    rc = lib.sv_png_assemble_batch(C.byref(plan), n, VP(*[s.ctypes.data for s in streams]), VP(*[b[1].ctypes.data for b in bands]), VP(*[b[2].ctypes.data for b in bands]),
                                   VP(*[o.ctypes.data for o in outs]), (C.c_size_t * n)(*caps), sizes, 2, status)
    assert rc == BUFFER and list(status) == [0, 0, BUFFER, 0] and sizes[2] == len(singles[2])


def test_refusals(lib):
    from sudoku_vision_amd._native import PngEnc
    plan = PngEnc()
    good = (20, 16, 3, 1, 0, 0)
    assert lib.sv_png_encode_plan(*good, C.byref(plan)) == 0
    for args in ((0, 16, 3, 1, 0, 0), (20, 0, 3, 1, 0, 0), (-1, 16, 3, 1, 0, 0), (65536, 16, 1, 1, 0, 0), (20, 65536, 3, 1, 0, 0), (20, 16, 2, 1, 0, 0), (20, 16, 4, 1, 0, 0),
                 (20, 16, 3, -1, 0, 0), (20, 16, 3, 6, 0, 0), (20, 16, 3, 1, -1, 0), (20, 16, 3, 1, 3, 0), (20, 16, 3, 1, 0, -1), (20, 16, 3, 1, 0, 513),
                 (20000, 16, 3, 1, 0, 2)):
        assert lib.sv_png_encode_plan(*args, C.byref(plan)) == BAD_ARG, args
    assert lib.sv_png_encode_plan(*good, None) == BAD_ARG
    assert lib.sv_png_encode_plan(21845, 2, 3, 1, 0, 0, C.byref(plan)) == UNSUPPORTED       # a row no band holds
    assert lib.sv_png_encode_plan(21844, 2, 3, 1, 0, 0, C.byref(plan)) == 0 and plan.band_rows == 1 and plan.bands == 2
    # automatic bands: about 32 KB, whole rows, at most 512 rows
    assert lib.sv_png_encode_plan(1920, 1080, 3, 1, 0, 0, C.byref(plan)) == 0
    assert plan.row_bytes == 5761 and 32768 <= plan.band_rows * plan.row_bytes <= 35000 and plan.bands == -(-1080 // plan.band_rows)
    assert lib.sv_png_encode_plan(1, 5000, 1, 1, 0, 0, C.byref(plan)) == 0 and plan.band_rows == 512 and plan.bands == 10
    assert lib.sv_png_encode_plan(20, 16, 3, 1, 0, 40, C.byref(plan)) == 0 and plan.band_rows == 16 and plan.bands == 1      # no more rows than the image

    img = R.content("synthetic", 16, 20)
    plan = make_plan(lib, 20, 16, 3, 4)
    stream, lens, adlers = zlib_bands(img, plan)
    rc, data = assemble(lib, plan, stream, lens, adlers)
    assert rc == 0
    rc, need = assemble(lib, plan, stream, lens, adlers, cap=len(data) - 1)
    assert rc == BUFFER and need == len(data)
    assert assemble(lib, plan, stream, lens, adlers, cap=len(data)) == (0, data)
    long_band = lens.copy()
    long_band[1] = plan.band_rows * plan.row_bytes + 11
    assert assemble(lib, plan, stream + bytes(1000), long_band, adlers)[0] == BAD_ARG
    bad_adler = adlers.copy()
    bad_adler[0] = 0xFFF1FFF1                                           # 65521 in both halves: not a residue
    assert assemble(lib, plan, stream, lens, bad_adler)[0] == BAD_ARG
    for edit in ("bands", "row_bytes", "slot_bytes", "stream_bound", "out_bound", "channels", "band_rows"):
        bad = PngEnc.from_buffer_copy(plan)
        setattr(bad, edit, getattr(bad, edit) + 1)
        assert assemble(lib, bad, stream, lens, adlers)[0] == BAD_ARG, edit
    size = C.c_size_t()
    out = np.zeros(int(plan.out_bound), np.uint8)
    buf = np.frombuffer(stream, np.uint8)
    for k in range(6):
        args = [C.byref(plan), buf.ctypes.data, lens.ctypes.data, adlers.ctypes.data, out.ctypes.data, out.size, C.byref(size)]
        if k == 5:
            continue                                                    # out_cap is a number
        args[k if k < 5 else 6] = None
        assert lib.sv_png_assemble(*args) == BAD_ARG
    assert lib.sv_png_assemble(C.byref(plan), buf.ctypes.data, lens.ctypes.data, adlers.ctypes.data, out.ctypes.data, out.size, None) == BAD_ARG
    assert lib.sv_png_deflate_bgr_u8(None, C.byref(plan), None, 1, 60, 0, None, None, None, None, None) == BAD_ARG
