"""Grayscale JPEG read, host part through the C ABI (no GPU): the luma-only mode of the entropy decoder (csrc/host_jpeg.cpp:
sv_jpeg_parse_luma, sv_jpeg_entropy_decode_luma, _luma_sparse, _luma_batch) against the full decode's Y blocks, block for block; that chroma
does not reach the output; that every stream the full decode refuses is refused with the same status and reason; and that buffers of exactly
the stated size are not overrun (a guard word after each)."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_gray_ref as G
import test_jpeg_crafted as T
from test_jpeg import encode, host, synth_image  # noqa: F401  (host: fixture)
from test_jpeg_gray_ref import SUBS, gray_file, gray_files, photo

GUARD16, GUARD32, GUARD64 = 0x5A5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


def restart_files():
    """restart intervals of 1 and 3 MCUs and of one MCU row, on partial-MCU sizes"""
    out = []
    for sub in SUBS:
        for kw in (dict(restart_marker_blocks=1), dict(restart_marker_blocks=3), dict(restart_marker_rows=1)):
            out.append(((sub, tuple(kw.items())), gray_file(53, 37, sub, 85, **kw)))
    return out


def lib_and_native():
    from sudoku_vision_amd import _native
    return _native.lib(), _native


def full_luma_blocks(host, data, threads=1):
    """Y's blocks of the existing full decode, rearranged into the luma-only record order; and Y's quantiser steps"""
    info, coef, quant = host.jpeg_entropy_decode(data, threads=threads)
    return G.scan_order(G.luma_blocks(coef, info.width, info.height, info.h_samp, info.v_samp), info.h_samp, info.v_samp), quant[0]


def check_luma_equals_full(host, data, what, threads=1):
    want, wq = full_luma_blocks(host, data)
    full = host.jpeg_parse(data)
    info, coef, quant = host.jpeg_entropy_decode_luma(data, threads=threads)
    mcus = -(-full.width // (8 * full.h_samp)) * -(-full.height // (8 * full.v_samp))
    assert info.coef_count == 64 * mcus * full.h_samp * full.v_samp == want.size, what
    assert (coef.reshape(-1, 64) == want).all() and (quant == wq).all(), what
    for f in ("width", "height", "out_width", "out_height", "components", "h_samp", "v_samp", "orientation", "restart_interval"):
        assert getattr(info, f) == getattr(full, f), (what, f)
    if full.components == 1:
        assert info.coef_count == full.coef_count and info.sparse_capacity == full.sparse_capacity
    else:
        assert info.coef_count < full.coef_count and info.sparse_capacity <= full.sparse_capacity
    info2, masks, offs, vals, quant2 = host.jpeg_entropy_decode_luma_sparse(data, threads=threads)
    assert info2.coef_count == info.coef_count and len(masks) == len(want) and len(vals) <= info2.sparse_capacity <= info2.coef_count, what
    assert (T.densify(info2, masks, offs, vals).reshape(-1, 64) == want).all() and (quant2 == wq).all(), what


@pytest.mark.parametrize("sub", SUBS)
def test_luma_decode_equals_y_of_full_decode(host, sub):
    for what, data in gray_files(sub):
        check_luma_equals_full(host, data, what)


def test_luma_decode_restart_intervals(host):
    for what, data in restart_files():
        assert host.jpeg_parse(data).restart_interval > 0
        for threads in (1, 3):
            check_luma_equals_full(host, data, what, threads)


def test_luma_decode_photo(host):
    check_luma_equals_full(host, photo(), "sample_4.jpg", threads=1)
    info = host.jpeg_parse_luma(photo())
    assert info.coef_count == 64 * 171 * 228 * 4                                     # 2736 x 3648 at 4:2:0: two thirds of the full count
    assert 3 * info.coef_count == 2 * host.jpeg_parse(photo()).coef_count


def test_non_interleaved_scans(host):
    """a file with one scan per component: Y's own scan walks Y's block grid, not the MCU grid, and leaves the MCU padding blocks zero"""
    import sv_oracle as o
    for sub in (2, 1, 0):
        data = encode(synth_image(37, 53, 9), quality=85, subsampling=sub)
        info, coef, quant = host.jpeg_entropy_decode(data)                            # Pillow writes one interleaved scan: re-code its coefficients
        split = _three_scans(coef, quant, info)
        assert split.count(b"\xff\xda") >= 3 and Image.open(io.BytesIO(split)).size == (53, 37)
        assert (G.pil_gray(split, 1) == G.pil_gray(data, 1)).all()                    # libjpeg reads the same luma from both
        assert (host.jpeg_entropy_decode(split)[1] == o.jpeg_coefficients(split)[0]).all()
        check_luma_equals_full(host, split, ("three scans", sub))
        assert (G.decode_file(split, 1) == G.pil_gray(split, 1)).all()


def _three_scans(coef, quant, info):
    """the file of (coef, quant) with one non-interleaved scan per component (each over the component's own ceil(size / 8) block grid)"""
    import jpeg_craft as J
    W, H, hs, vs = info.width, info.height, info.h_samp, info.v_samp
    whole = J.write_jpeg(coef, quant.astype(np.int64), W, H, "4:2:0" if (hs, vs) == (2, 2) else "4:2:2" if hs == 2 else "4:4:4")
    head = whole[:whole.index(b"\xff\xda")]
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    out, off = bytearray(head), 0
    for c, (h, v) in enumerate([(hs, vs), (1, 1), (1, 1)]):
        bw, bh = mcux * h, mcuy * v
        blocks = coef[off:off + 64 * bw * bh].reshape(bh, bw, 64)
        off += 64 * bw * bh
        cw, chh = -(-(-(-W * h // hs)) // 8), -(-(-(-H * v // vs)) // 8)
        own = np.ascontiguousarray(blocks[:chh, :cw]).reshape(-1, 64)
        gray = J.write_jpeg(own, np.ones((1, 64), np.int64), 8 * cw, 8 * chh, "gray")        # a gray file's scan is this component's scan with tables 0
        bits = gray[gray.index(b"\xff\xda") + 10:-2]
        if c:                                                                          # chroma uses tables 1: re-code through a colour file of one row
            bits = _recode_chroma(own, cw, chh)
        out += b"\xff\xda" + (8).to_bytes(2, "big") + bytes([1, c + 1, 0x11 if c else 0x00, 0, 63, 0]) + bits
    return bytes(out + b"\xff\xd9")


def _recode_chroma(blocks, cw, chh):
    """entropy-coded bytes of `blocks` as a single-component scan with the chrominance tables"""
    import jpeg_craft as J
    dc, ac = J._huff_codes(*J.STD_HUFFMAN[(0, 1)]), J._huff_codes(*J.STD_HUFFMAN[(1, 1)])
    w, pred = J._BitWriter(), 0
    for blk in blocks.astype(np.int64):
        zz = blk[J._ZZ]
        diff, pred = int(zz[0] - pred), int(zz[0])
        size = abs(diff).bit_length()
        w.put(*dc[size])
        if size:
            w.put(diff if diff > 0 else diff + (1 << size) - 1, size)
        run = 0
        for k in range(1, 64):
            a = int(zz[k])
            if a == 0:
                run += 1
                continue
            while run > 15:
                w.put(*ac[0xF0])
                run -= 16
            size = abs(a).bit_length()
            w.put(*ac[run << 4 | size])
            w.put(a if a > 0 else a + (1 << size) - 1, size)
            run = 0
        if run:
            w.put(*ac[0])
    return w.flush()


def test_chroma_does_not_reach_the_output(host):
    """two crafted files with identical Y and different chroma: identical luma-only blocks.  Without restart intervals the compact records
    are identical word for word; with them each interval appends to its own stretch of the value stream, sized from the interval's bytes, so
    a block's offset may move with the chroma's size -- its mask and its values may not."""
    rs = np.random.RandomState(5)
    for sampling in ("4:4:4", "4:2:2", "4:2:0"):
        (ybw, ybh), (cbw, cbh), _ = T.grids(37, 29, sampling)
        y = rs.randint(-30, 31, (ybw * ybh, 64))
        quant = rs.randint(1, 9, (3, 64))
        want = G.scan_order(y.reshape(ybh, ybw, 64), *T.SAMPLINGS[sampling][1:])
        for interval in (0, 2):
            files = []
            for seed in (1, 2):
                cs = np.random.RandomState(seed)
                chroma = [cs.randint(-60 * seed, 60 * seed + 1, (cbw * cbh, 64)) for _ in range(2)]
                files.append(T.craft(np.concatenate([y] + chroma), quant, 37, 29, sampling, restart_interval=interval))
            assert files[0].data != files[1].data
            a, b = (host.jpeg_entropy_decode_luma(f.data) for f in files)
            assert (a[1] == b[1]).all() and (a[2] == b[2]).all() and (a[2] == quant[0]).all()
            assert (a[1].reshape(-1, 64) == want).all()
            sa, sb = (host.jpeg_entropy_decode_luma_sparse(f.data) for f in files)
            assert (sa[1] == sb[1]).all() and (sa[4] == sb[4]).all()
            assert (T.densify(*sa[:4]).reshape(-1, 64) == want).all() and (T.densify(*sb[:4]).reshape(-1, 64) == want).all()
            if interval == 0:
                assert (sa[2] == sb[2]).all() and (sa[3] == sb[3]).all(), sampling


def refused_streams():
    good = gray_file(33, 17, 2, 95)
    sof = good.index(b"\xff\xc0")
    out = {"progressive": encode(synth_image(32, 32, 1), quality=80, progressive=True),
           "png": b"\x89PNG\r\n\x1a\n" + b"\0" * 64, "empty": b"", "soi only": b"\xff\xd8", "soi eoi": b"\xff\xd8\xff\xd9"}
    cmyk = io.BytesIO()
    Image.fromarray(synth_image(16, 16, 2)).convert("CMYK").save(cmyk, "JPEG")
    out["cmyk"] = cmyk.getvalue()
    patch = lambda at, v: good[:at] + bytes([v]) + good[at + 1:]
    out["12-bit"] = patch(sof + 4, 12)
    out["arithmetic"] = patch(sof + 1, 0xC9)
    out["lossless"] = patch(sof + 1, 0xC3)
    out["sampling 4x1"] = patch(sof + 11, 0x41)
    out["sampling 1x2"] = patch(sof + 11, 0x12)
    out["chroma 2x1"] = patch(sof + 14, 0x21)
    out["zero height"] = good[:sof + 5] + b"\0\0" + good[sof + 7:]
    out["undefined quant table"] = patch(sof + 15, 3)                                 # Cb's table: Y-only output, yet the full decode's refusal stands
    sos = good.index(b"\xff\xda")
    out["undefined huffman table"] = patch(sos + 8, 0x33)                             # Cb's tables in the scan header
    out["unknown scan component"] = patch(sos + 9, 9)
    out["spectral selection"] = patch(sos + 12, 5)
    dht = good.index(b"\xff\xc4")
    out["over-subscribed huffman"] = patch(dht + 5, 200)
    for cut in list(range(0, sos + 16)) + [sos + 40]:
        out[f"cut at {cut}"] = good[:cut]
    return out


def test_refusals_are_the_full_decodes_refusals(host):
    """status and reason: parse, dense and compact entries of both modes on every stream; whatever the full decode answers, the luma mode answers"""
    lib, native = lib_and_native()
    refused = 0
    for name, data in refused_streams().items():
        info, linfo = native.JpegInfo(), native.JpegInfo()
        a = lib.sv_jpeg_parse(data, len(data), C.byref(info))
        ea = lib.sv_last_error() if a else b""
        b = lib.sv_jpeg_parse_luma(data, len(data), C.byref(linfo))
        eb = lib.sv_last_error() if b else b""
        assert a == b and ea == eb, (name, a, b, ea, eb)
        coef = np.zeros(max(64, info.coef_count if a == 0 else 64), np.int16)
        cap = max(64, info.sparse_capacity if a == 0 else 64)
        masks, offs, vals = np.zeros(coef.size // 64, np.uint64), np.zeros(coef.size // 64, np.uint32), np.zeros(cap, np.int16)
        quant, used = np.zeros(192, np.uint16), C.c_long()
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        for full, luma, args in ((lib.sv_jpeg_entropy_decode, lib.sv_jpeg_entropy_decode_luma, (p(coef), p(quant), 1)),
                                 (lib.sv_jpeg_entropy_decode_sparse, lib.sv_jpeg_entropy_decode_luma_sparse, (p(masks), p(offs), p(vals), cap, C.byref(used), p(quant), 1))):
            a = full(data, len(data), *args)
            ea = lib.sv_last_error() if a else b""
            b = luma(data, len(data), *args)
            eb = lib.sv_last_error() if b else b""
            assert a == b and ea == eb, (name, a, b, ea, eb)
            refused += a != 0
    assert refused > 100
    for name, status in (("progressive", -4), ("cmyk", -4), ("12-bit", -4), ("arithmetic", -4), ("sampling 4x1", -4), ("png", -1), ("undefined quant table", -1)):
        data = refused_streams()[name]
        assert lib.sv_jpeg_parse_luma(data, len(data), C.byref(native.JpegInfo())) in (status, 0)
        assert lib.sv_jpeg_entropy_decode_luma(data, len(data), coef.ctypes.data_as(C.c_void_p), quant.ctypes.data_as(C.c_void_p), 1) == status, name


def test_truncated_scans_decode_like_the_full_decode(host):
    """a file cut inside its entropy-coded data is not refused (libjpeg: insufficient data reads as zero blocks); the luma mode returns the Y
    blocks the full decode returns for the same cut"""
    for sub, kw in ((2, {}), (1, dict(restart_marker_blocks=2)), ("L", {})):
        data = gray_file(53, 37, sub, 95, **kw)
        start = data.index(b"\xff\xda") + 14
        from sudoku_vision_amd._native import NativeError
        decoded = 0
        for cut in range(start, len(data), 23):
            try:
                host.jpeg_entropy_decode(data[:cut])
            except NativeError as e:                                                   # too few restart intervals left: a refusal of both modes
                with pytest.raises(NativeError) as luma:
                    host.jpeg_entropy_decode_luma(data[:cut])
                assert str(luma.value).split(": ", 1)[1] == str(e).split(": ", 1)[1]
                continue
            check_luma_equals_full(host, data[:cut], (sub, cut))
            decoded += 1
        assert decoded > 5


def exact_buffers(info):
    """numpy buffers of exactly the stated sizes + one guard word each, and the guards' positions"""
    nb = info.coef_count // 64
    coef = np.full(info.coef_count + 1, GUARD16, np.uint16)
    masks, offs = np.full(nb + 1, GUARD64, np.uint64), np.full(nb + 1, GUARD32, np.uint32)
    vals = np.full(info.sparse_capacity + 1, GUARD16, np.uint16)
    quant = np.full(64 + 1, GUARD16, np.uint16)
    return coef, masks, offs, vals, quant


def guards_intact(*arrays):
    return all(int(a[-1]) == {2: GUARD16, 4: GUARD32, 8: GUARD64}[a.itemsize] for a in arrays)


def test_exact_buffers_are_not_overrun(host):
    lib, native = lib_and_native()
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    files = [d for sub in SUBS for _, d in gray_files(sub)] + [d for _, d in restart_files()]
    for data in (gray_file(53, 37, 2, 95), gray_file(53, 37, 0, 30), gray_file(33, 17, "L", 95)):      # cut inside the entropy-coded data
        scan = data.index(b"\xff\xda") + 14
        files += [data[:scan + (len(data) - scan) // 2], data[:scan + 3]]
    for data in files:
        info = host.jpeg_parse_luma(data)
        coef, masks, offs, vals, quant = exact_buffers(info)
        assert lib.sv_jpeg_entropy_decode_luma(data, len(data), p(coef), p(quant), 2) == 0
        assert guards_intact(coef, quant)
        used = C.c_long(-1)
        quant[:] = GUARD16
        assert lib.sv_jpeg_entropy_decode_luma_sparse(data, len(data), p(masks), p(offs), p(vals), info.sparse_capacity, C.byref(used), p(quant), 2) == 0
        assert guards_intact(masks, offs, vals, quant) and 0 <= used.value <= info.sparse_capacity
        # one value short of the stated capacity: SV_ERR_BUFFER or a decode that still fits, never a write past the end
        rc = lib.sv_jpeg_entropy_decode_luma_sparse(data, len(data), p(masks), p(offs), p(vals), max(0, info.sparse_capacity - 1), C.byref(used), p(quant), 1)
        assert rc in (0, -6) and guards_intact(masks, offs, vals, quant)


def test_batch_entry(host):
    """sv_jpeg_entropy_decode_luma_batch, dense and compact, mixed samplings: each image as the single-image entry decodes it, in exact
    buffers; a refused image fails the batch with its own status and leaves the others decoded"""
    lib, native = lib_and_native()
    datas = [gray_file(53, 37, 2, 95), gray_file(33, 17, "L", 30), gray_file(17, 17, 1, 95), gray_file(9, 9, 0, 30)]
    n = len(datas)
    infos = [host.jpeg_parse_luma(d) for d in datas]
    bufs = [exact_buffers(i) for i in infos]
    quants = np.full(64 * n + 1, GUARD16, np.uint16)
    VP = C.c_void_p * n
    arr = lambda k: VP(*[b[k].ctypes.data for b in bufs])
    sizes, status = (C.c_size_t * n)(*[len(d) for d in datas]), (C.c_int * n)()
    raw = (C.c_char_p * n)(*datas)
    q = quants.ctypes.data_as(C.c_void_p)
    assert lib.sv_jpeg_entropy_decode_luma_batch(raw, sizes, n, arr(0), None, None, None, None, None, q, 3, status) == 0
    caps, used = (C.c_long * n)(*[i.sparse_capacity for i in infos]), (C.c_long * n)()
    assert lib.sv_jpeg_entropy_decode_luma_batch(raw, sizes, n, None, arr(1), arr(2), arr(3), caps, used, q, 3, status) == 0
    assert int(quants[-1]) == GUARD16
    for i, d in enumerate(datas):
        want, wq = full_luma_blocks(host, d)
        coef, masks, offs, vals, _ = bufs[i]
        assert guards_intact(coef, masks, offs, vals)
        assert (coef[:-1].view(np.int16).reshape(-1, 64) == want).all() and (quants[64 * i:64 * i + 64] == wq).all()
        assert (T.densify(infos[i], masks[:-1], offs[:-1], vals[:used[i]].view(np.int16)).reshape(-1, 64) == want).all()
    bad = encode(synth_image(32, 32, 1), quality=80, progressive=True)
    raw2 = (C.c_char_p * 2)(datas[1], bad)
    sizes2, status2 = (C.c_size_t * 2)(len(datas[1]), len(bad)), (C.c_int * 2)()
    coefs2 = (C.c_void_p * 2)(bufs[1][0].ctypes.data, bufs[0][0].ctypes.data)
    assert lib.sv_jpeg_entropy_decode_luma_batch(raw2, sizes2, 2, coefs2, None, None, None, None, None, q, 2, status2) == -4
    assert list(status2) == [0, -4]
