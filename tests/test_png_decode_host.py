"""CPU: the PNG decoder's host half (csrc/host_png.cpp: sv_png_parse, sv_png_inflate, _batch) through sudoku_vision_amd.host.  The inflater is the
project's own, so every stream here is inflated by zlib.decompress too and the bytes compared; the malformed streams are built by hand, bit by
bit, and each must come back as a status (NativeError), never a crash, with a valid call succeeding right after."""
import os
import struct
import zlib

import numpy as np
import pytest

import png_craft as K
import png_encode_ref as R


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as g
    import sudoku_vision_amd as sva
    if not os.path.exists(sva._native.LIB_PATH):
        g.build()
    from sudoku_vision_amd import host
    return host


def gray_file(payload, raw_len, split=None, **kw):
    """an 8-bit gray file of ONE row of raw_len - 1 pixels around `payload`: any byte string whose first byte is a filter type is its filtered image"""
    return K.assemble(raw_len - 1, 1, 0, 8, payload, split=split, **kw)


def rows_file(payload, width, height, split=None):
    return K.assemble(width, height, 0, 8, payload, split=split)


def inflate_ok(host, data, want):
    info, filtered, row_filter = host.png_inflate(data)
    assert filtered.tobytes() == want
    row = 1 + info.row_bytes
    assert row_filter.tolist() == [want[r * row] for r in range(info.height)]


def refused(host, data, why):
    """SV_ERR_BAD_ARG with the reason `why` in sv_last_error's text: a malformed case must fail for ITS reason, not for another"""
    import re
    from sudoku_vision_amd._native import NativeError
    with pytest.raises(NativeError, match="SV_ERR_BAD_ARG.*" + re.escape(why)):
        host.png_inflate(data)
    inflate_ok(host, GOOD, GOOD_RAW)                                    # the library is as usable as before


GOOD_RAW = b"\x01" + bytes(range(40))
GOOD = gray_file(zlib.compress(GOOD_RAW), len(GOOD_RAW))


def image_bytes(height, width, seed, noise=False):
    """filtered bytes of an 8-bit gray image whose rows carry filter types 0..4"""
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 256, (height, 1 + width)) if noise else (np.arange(height * (1 + width)).reshape(height, -1) // 7 * 13) % 251
    a = a.astype(np.uint8)
    a[:, 0] = rs.randint(0, 5, height)
    return a.tobytes()


@pytest.mark.parametrize("level", [0, 1, 6, 9])
@pytest.mark.parametrize("strategy", ["default", "fixed", "huffman_only", "rle", "filtered"])
@pytest.mark.parametrize("wbits", [9, 15])
def test_matches_zlib(host, level, strategy, wbits):
    strat = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "huffman_only": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE, "filtered": zlib.Z_FILTERED}[strategy]
    for H, W, noise in ((60, 99, False), (33, 200, True), (1, 1, False)):
        raw = image_bytes(H, W, H + level, noise)
        payload = K.deflate(raw, level, strat, wbits)
        assert zlib.decompress(payload) == raw
        inflate_ok(host, rows_file(payload, W, H), raw)


def test_long_distances_long_matches_and_stored_blocks(host):
    rs = np.random.RandomState(3)
    # a long way back, as far as zlib's own deflater goes (w_size - 262 = 32,506): 32,400 random bytes, then their first 300 again.  The match at
    # distance 32,768 itself is hand-built in test_distance_32768 below.
    block = rs.randint(0, 256, 32400, dtype=np.uint8).tobytes()
    raw = b"\x00" + block + block[:300]
    W = len(raw) - 1
    payload = K.deflate(raw, 9)
    assert len(payload) < len(K.deflate(b"\x00" + block + rs.randint(0, 256, 300, dtype=np.uint8).tobytes(), 9)) - 200        # the repeat was found
    inflate_ok(host, rows_file(payload, W, 1), raw)
    # length-258 matches at distance 1
    raw = b"\x00" + bytes([7]) * 5000
    inflate_ok(host, rows_file(K.deflate(raw, 6), 5000, 1), raw)
    # incompressible data in stored blocks, more than 65,535 bytes so several
    a = rs.randint(0, 256, (2, 35000), dtype=np.uint8)
    a[:, 0] = (2, 4)
    raw = a.tobytes()
    payload = K.deflate(raw, 0)
    assert len(payload) > 70000 + 10
    inflate_ok(host, rows_file(payload, 34999, 2), raw)
    payload = K.deflate(raw, 6)
    inflate_ok(host, rows_file(payload, 34999, 2), raw)
    # an empty stored block mid-stream
    c = zlib.compressobj(6)
    payload = c.compress(raw[:3000]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(raw[3000:]) + c.flush()
    assert b"\x00\x00\xff\xff" in payload
    inflate_ok(host, rows_file(payload, 34999, 2), raw)


def test_idat_split_everywhere(host):
    raw = image_bytes(12, 17, 1)
    payload = K.deflate(raw, 6)
    assert len(payload) < 200
    for cut in range(len(payload) + 1):
        inflate_ok(host, rows_file(payload, 17, 12, split=[cut]), raw)
    inflate_ok(host, rows_file(payload, 17, 12, split=[0, 0, 1, 0, 1, 1, 0]), raw)
    inflate_ok(host, rows_file(payload, 17, 12, split=[1] * len(payload)), raw)
    for strategy in (zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY):
        p = K.deflate(raw, 6, strategy)
        inflate_ok(host, rows_file(p, 17, 12, split=[1] * len(p)), raw)
    p = K.deflate(raw, 0)
    for cut in range(len(p) + 1):
        inflate_ok(host, rows_file(p, 17, 12, split=[cut]), raw)


def test_k18_assembled_files(host):
    """the files the encoder's host half assembles from bands (tests/test_png_encode_host.py's construction: raw Z_RLE streams ended by a sync flush)"""
    import ctypes as C
    from sudoku_vision_amd import _native
    lib = _native.lib()
    for gray in (False, True):
        img = R.content("synthetic", 21, 30, gray)
        plan = _native.PngEnc()
        assert lib.sv_png_encode_plan(30, 21, 1 if gray else 3, 1, 0, 5, C.byref(plan)) == 0
        f = R.filtered(img, "sub")
        per = plan.band_rows * plan.row_bytes
        parts, adlers = [], []
        for b in range(plan.bands):
            c = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
            parts.append(c.compress(f[b * per:(b + 1) * per]) + c.flush(zlib.Z_SYNC_FLUSH))
            adlers.append(zlib.adler32(f[b * per:(b + 1) * per]))
        stream = np.frombuffer(b"".join(parts) + b"\0", np.uint8)
        lens, ad = np.array([len(p) for p in parts], np.uint32), np.array(adlers, np.uint32)
        out, size = np.zeros(int(plan.out_bound), np.uint8), C.c_size_t()
        assert lib.sv_png_assemble(C.byref(plan), stream.ctypes.data, lens.ctypes.data, ad.ctypes.data, out.ctypes.data, out.size, C.byref(size)) == 0
        data = out[:size.value].tobytes()
        info, filtered, rf = host.png_inflate(data)
        assert (info.width, info.height, info.bit_depth, info.color_type) == (30, 21, 8, 0 if gray else 2)
        assert filtered.tobytes() == f and rf.tolist() == [1] * 21


# ---- hand-built deflate streams ------------------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.bits = []

    def put(self, value, n):                                           # LSB first: header fields and extra bits
        self.bits += [(value >> i) & 1 for i in range(n)]
        return self

    def code(self, value, n):                                          # MSB first: Huffman codes
        self.bits += [(value >> i) & 1 for i in range(n - 1, -1, -1)]
        return self

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def canonical(lengths):
    """{symbol: (code, length)} of a canonical Huffman code"""
    code, out = 0, {}
    for n in range(1, 16):
        for s, l in enumerate(lengths):
            if l == n:
                out[s] = (code, n)
                code += 1
        code <<= 1
    return out


CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def dynamic_block(cl_lengths, length_symbols, hlit, hdist, body, last=1):
    """a dynamic block: cl_lengths: the 19 code-length-code lengths; length_symbols: [(symbol, extra value, extra bits)] that spell the HLIT + HDIST
    lengths; body(bits): writes the block's data"""
    w = Bits().put(last, 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(19 - 4, 4)
    for s in CL_ORDER:
        w.put(cl_lengths[s], 3)
    cl = canonical(cl_lengths)
    for sym, extra, nbits in length_symbols:
        w.code(*cl[sym])
        w.put(extra, nbits)
    body(w)
    return w


def zwrap(deflate_bytes, raw):
    return b"\x78\x9c" + deflate_bytes + struct.pack(">I", zlib.adler32(raw))


def check_both(host, payload, raw):
    assert zlib.decompress(payload) == raw                             # the hand-built stream is one zlib accepts
    inflate_ok(host, gray_file(payload, len(raw)), raw)


def test_repeat_runs_from_literals_into_distances(host):
    """HLIT = 259, HDIST = 4.  Literal/length lengths: 'A' (65), 256, 257, 258 = 2 bits each (complete); distance lengths 2, 2, 2, 2 (complete).  The
    lengths are spelled: 65 zeros (18), '2', 190 zeros (18, 18), '2' for 256, then ONE code 16 repeating it six times: 257, 258 and distances
    0..3 -- the repeat runs from the literal alphabet into the distance alphabet.  The filter byte comes from a stored block in front."""
    cl = [0] * 19
    cl[0], cl[1], cl[2], cl[16], cl[18] = 2, 2, 2, 3, 3               # 3/4 + 2/8: complete
    hlit, hdist = 259, 4
    syms = [(18, 65 - 11, 7), (2, 0, 0), (18, 138 - 11, 7), (18, 190 - 138 - 11, 7), (2, 0, 0), (16, 6 - 3, 2)]
    lit = canonical([0] * 65 + [2] + [0] * 190 + [2, 2, 2])
    dist = canonical([2, 2, 2, 2])

    def body(w):
        w.code(*lit[65]).code(*lit[65]).code(*lit[65])
        w.code(*lit[257]).code(*dist[1])                                # length 3, distance 2
        w.code(*lit[258]).code(*dist[0])                                # length 4, distance 1
        w.code(*lit[256])
    raw = b"\x00" + b"A" * 10
    stored = Bits().put(0, 1).put(0, 2).bytes() + struct.pack("<HH", 1, 0xFFFE) + b"\x00"
    payload = zwrap(stored + dynamic_block(cl, syms, hlit, hdist, body).bytes(), raw)
    check_both(host, payload, raw)


def test_fifteen_bit_codes_and_single_distance_code(host):
    # literal/length lengths 1, 2, ..., 14, 15, 15 on symbols 'a'.. and 256: a complete code whose longest codes take the second-level table
    lengths = [0] * 258
    symbols = list(range(97, 97 + 14)) + [256, 257]
    for s, l in zip(symbols, list(range(1, 15)) + [15, 15]):
        lengths[s] = l
    cl = [0] * 19
    for s in range(16):
        cl[s] = 5                                                      # 16 codes of 5 bits + 17, 18 of 2 bits: 16/32 + 2/4 = 1
    cl[17], cl[18] = 2, 2
    cl[16] = 0
    syms = []
    at = 0
    spelled = lengths + [1]                                            # HDIST = 1: a single distance code of one bit, the incomplete code zlib accepts
    while at < len(spelled):
        if spelled[at] == 0:
            run = 0
            while at + run < len(spelled) and spelled[at + run] == 0 and run < 138:
                run += 1
            if run >= 11:
                syms.append((18, run - 11, 7))
            elif run >= 3:
                syms.append((17, run - 3, 3))
            else:
                syms += [(0, 0, 0)] * run
            at += run
        else:
            syms.append((spelled[at], 0, 0))
            at += 1
    lit, dist = canonical(lengths), canonical([1])

    def body(w):
        for s in symbols[:14]:
            w.code(*lit[s])
        w.code(*lit[257]).code(*dist[0])                                # length 3 at distance 1, through a 15-bit code
        w.code(*lit[256])
    raw = b"\x00" + bytes(symbols[:14]) + bytes([symbols[13]]) * 3
    stored = Bits().put(0, 1).put(0, 2).bytes() + struct.pack("<HH", 1, 0xFFFE) + b"\x00"
    payload = zwrap(stored + dynamic_block(cl, syms, 258, 1, body).bytes(), raw)
    check_both(host, payload, raw)


def stored_block(last, data):
    return bytes([last]) + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data


def far_match(head):
    """stored `head`, then a fixed block: length 3 at distance 32,768 -- distance code 29, whose 13 extra bits are all ones -- and the end of block"""
    w = Bits().put(1, 1).put(1, 2).code(1, 7).code(29, 5).put(8191, 13).code(0, 7)
    return stored_block(0, head) + w.bytes()


def test_distance_32768(host):
    """zlib's deflater never writes a distance above 32,506, so the window's far edge is built by hand: 32,768 bytes out, then a match that reaches
    back to the very first of them; and one byte fewer out, where the same match reaches before the start"""
    head = b"\x00" + np.random.RandomState(4).randint(0, 256, 32767, dtype=np.uint8).tobytes()
    raw = head + head[:3]
    check_both(host, zwrap(far_match(head), raw), raw)
    short = head[:-1]
    bad = zwrap(far_match(short), short + short[:3])
    with pytest.raises(zlib.error):
        zlib.decompress(bad)
    refused(host, gray_file(bad, len(short) + 3), "a distance before the start of the output")


def test_malformed_streams(host):
    raw = GOOD_RAW
    good = zlib.compress(raw, 6)
    n = len(raw)

    def z(deflate):
        return gray_file(b"\x78\x9c" + deflate + struct.pack(">I", zlib.adler32(raw)), n)
    stored = stored_block
    assert host.png_inflate(z(stored(1, raw)))[1].tobytes() == raw
    # truncated at every length
    for cut in range(len(good)):
        refused(host, gray_file(good[:cut], n), "truncated input")
    # the zlib header
    refused(host, gray_file(b"\x79\x9c" + good[2:], n), "the method is not deflate")          # CM 9
    refused(host, gray_file(b"\x88\x1c" + good[2:], n), "a window above 32 K")                # window 64 K
    refused(host, gray_file(b"\x78\xbb" + good[2:], n), "a preset dictionary")                # FDICT (FCHECK right)
    refused(host, gray_file(b"\x78\x9d" + good[2:], n), "FCHECK")
    assert (0x78 * 256 + 0xbb) % 31 == 0 and (0x88 * 256 + 0x1c) % 31 == 0
    refused(host, z(b"\x01" + struct.pack("<HH", n, n) + raw), "LEN is not the complement of NLEN")
    refused(host, z(Bits().put(1, 1).put(3, 2).bytes() + raw), "block type 3")
    # wrong Adler-32, short stream, long stream
    refused(host, gray_file(good[:-1] + bytes([good[-1] ^ 1]), n), "wrong Adler-32")
    refused(host, gray_file(zlib.compress(raw[:-1]), n), "fewer than the image's bytes")
    refused(host, gray_file(zlib.compress(raw + b"x"), n), "more than the image's bytes")
    refused(host, gray_file(zlib.compress(raw + bytes(100000)), n), "more than the image's bytes")    # a bomb stops at the image's size
    refused(host, z(stored(0, raw) + stored(1, b"xx")), "more than the image's bytes")
    # a distance before the start of the output: fixed block, literal 0, then length 3 at distance 2
    w = Bits().put(1, 1).put(1, 2).code(0x30, 8).code(1, 7).code(1, 5).code(0, 7)
    refused(host, z(w.bytes()), "a distance before the start of the output")
    # codes.  The code-length code: 0, 1, 2 in two bits, 16 and 18 in three (complete); the lengths are then spelled with it
    cl = [0] * 19
    cl[0], cl[1], cl[2], cl[16], cl[18] = 2, 2, 2, 3, 3
    body = lambda w: None
    zeros256 = [(18, 127, 7), (18, 256 - 138 - 11, 7)]                  # lengths 0 for the literals 0..255
    one, two = (1, 0, 0), (2, 0, 0)
    # HLIT 258, HDIST 2: 257 zeros, so 256 has no code; 257 and the distances 1, 1, 1
    refused(host, z(dynamic_block(cl, [(18, 127, 7), (18, 257 - 138 - 11, 7), one, one, one], 258, 2, body).bytes()), "no end-of-block code")
    # HLIT 259, HDIST 1: 256, 257, 258 all of length 1 -- three one-bit codes
    refused(host, z(dynamic_block(cl, zeros256 + [one, one, one, one], 259, 1, body).bytes()), "over-subscribed literal/length code")
    # HLIT 258, HDIST 2: 256, 257 of length 2 -- half the code space unused
    refused(host, z(dynamic_block(cl, zeros256 + [two, two, one, one], 258, 2, body).bytes()), "incomplete literal/length code")
    # HLIT 258, HDIST 3: a complete literal/length code 1, 1; distances 1, 1, 1 and 2, 2 (two codes of two bits: not the single one-bit code zlib accepts)
    refused(host, z(dynamic_block(cl, zeros256 + [one, one, one, one, one], 258, 3, body).bytes()), "over-subscribed distance code")
    refused(host, z(dynamic_block(cl, zeros256 + [one, one, two, two], 258, 2, body).bytes()), "incomplete distance code")
    refused(host, z(dynamic_block(cl, [(16, 0, 2)], 258, 2, body).bytes()), "a code-length repeat with no previous length")
    refused(host, z(dynamic_block(cl, [(18, 127, 7), (18, 127, 7)], 258, 2, body).bytes()), "a code-length repeat past HLIT + HDIST")          # 276 zeros, 260 lengths
    over = [0] * 19
    over[0], over[1], over[2], over[3], over[4] = 1, 1, 2, 2, 2
    refused(host, z(dynamic_block(over, [], 258, 2, body).bytes()), "over-subscribed code-length code")
    under = [0] * 19
    under[0], under[1] = 2, 2
    refused(host, z(dynamic_block(under, [], 258, 2, body).bytes()), "incomplete code-length code")
    # a filter byte above 4
    bad = b"\x05" + raw[1:]
    refused(host, gray_file(zlib.compress(bad), n), "filter type 5")


def test_batch_statuses(host):
    raw = image_bytes(9, 14, 2)
    good = rows_file(zlib.compress(raw), 14, 9)
    broken = rows_file(zlib.compress(raw)[:-3] + b"abc", 14, 9)
    for threads in (1, 4):
        infos, outs, rows, status = host.png_inflate_batch([good, broken, good], threads=threads)
        assert status.tolist() == [0, -1, 0] and outs[0].tobytes() == raw and outs[2].tobytes() == raw
    info = host.png_parse(good)
    from sudoku_vision_amd._native import NativeError
    with pytest.raises(NativeError, match="BUFFER"):
        host.png_inflate(good, info, np.empty(info.filtered_bytes - 1, np.uint8))


def test_parse_accepts_every_format(host):
    for color_type, depth in K.ALL_FORMATS:
        pal = K.random_palette(2) if color_type == 3 else None
        data = K.make_png(K.random_samples(3, 5, color_type, depth, limit=2 if pal is not None else None), color_type, depth, 0, palette=pal)
        info = host.png_parse(data)
        ch = K.CHANNELS[color_type]
        assert (info.width, info.height, info.bit_depth, info.color_type, info.interlace, info.channels) == (5, 3, depth, color_type, 0, ch)
        assert info.row_bytes == (5 * ch * depth + 7) // 8 and info.bpp == max(1, ch * depth // 8) and info.filtered_bytes == 3 * (1 + info.row_bytes)
        assert info.palette_entries == (2 if pal is not None else 0) and bytes(info.palette)[:6] == (pal.tobytes() if pal is not None else bytes(6))
    data = K.make_png(K.random_samples(2, 2, 2, 8), 2, 8, 0, before_idat=[(b"gAMA", bytes(4)), (b"tRNS", bytes(6))], after_idat=[(b"tIME", bytes(7))])
    assert host.png_parse(data).width == 2


def test_parse_refusals(host):
    from sudoku_vision_amd._native import NativeError
    raw = b"\x00\x07"
    z = zlib.compress(raw)
    ihdr = lambda w=1, h=1, d=8, t=0, c=0, f=0, i=0: R.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, d, t, c, f, i))
    idat, iend, sig = R.chunk(b"IDAT", z), R.chunk(b"IEND", b""), R.SIGNATURE
    assert host.png_parse(sig + ihdr() + idat + iend).filtered_bytes == 2

    def bad(data, what="BAD_ARG"):
        with pytest.raises(NativeError, match=what):
            host.png_parse(data)
        assert host.png_parse(sig + ihdr() + idat + iend).width == 1

    bad(b"\x89PNG\r\n\x1a\r" + ihdr() + idat + iend)                   # signature
    bad(sig[:5])
    bad(sig + ihdr()[:-1] + b"\0" + idat + iend)                        # IHDR's CRC
    bad(sig + ihdr() + idat[:-1] + bytes([idat[-1] ^ 1]) + iend)        # IDAT's CRC
    bad(sig + idat + iend)                                              # no IHDR
    bad(sig + ihdr() + iend)                                            # no IDAT
    bad(sig + ihdr() + idat)                                            # no IEND
    bad(sig + ihdr() + idat[:10])                                       # a chunk that runs past the file
    bad(sig + idat + ihdr() + iend)                                     # out of order
    bad(sig + ihdr() + ihdr() + idat + iend)
    bad(sig + ihdr() + idat + R.chunk(b"tEXt", b"a\0b") + idat + iend)  # IDATs not consecutive
    bad(sig + ihdr(t=3) + idat + iend)                                  # no PLTE for colour type 3
    bad(sig + ihdr(t=3) + idat + R.chunk(b"PLTE", bytes(6)) + iend)     # PLTE after IDAT
    bad(sig + ihdr(t=3) + R.chunk(b"PLTE", bytes(7)) + idat + iend)     # not a multiple of 3
    bad(sig + ihdr(t=3) + R.chunk(b"PLTE", bytes(771)) + idat + iend)   # more than 256 entries
    bad(sig + ihdr(w=0) + idat + iend)
    bad(sig + ihdr(h=0) + idat + iend)
    bad(sig + ihdr(d=3) + idat + iend)
    bad(sig + ihdr(t=2, d=4) + idat + iend)
    bad(sig + ihdr(t=3, d=16) + idat + iend)
    bad(sig + ihdr(t=1) + idat + iend)
    bad(sig + ihdr(c=1) + idat + iend)
    bad(sig + ihdr(f=1) + idat + iend)
    bad(sig + ihdr(i=2) + idat + iend)
    bad(sig + ihdr() + R.chunk(b"ABCD", b"") + idat + iend)             # an unknown critical chunk
    bad(sig + ihdr(i=1) + idat + iend, "UNSUPPORTED")                   # Adam7
    bad(sig + ihdr(w=65536) + idat + iend, "UNSUPPORTED")
    bad(sig + ihdr(w=65535, h=65535, t=6, d=16) + idat + iend, "UNSUPPORTED")     # above 512 MiB of filtered bytes
    assert host.png_parse(sig + ihdr(t=3) + R.chunk(b"PLTE", bytes(768)) + idat + iend).palette_entries == 256
    assert host.png_parse(sig + ihdr() + R.chunk(b"abCd", b"xyz")[:-1] + b"\0" + idat + iend).width == 1      # an ancillary chunk's CRC is not read
