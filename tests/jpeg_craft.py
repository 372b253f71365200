"""A baseline JPEG writer for coefficients the tests choose themselves (tests/test_jpeg_crafted.py, tests/test_gpu_jpeg_crafted.py).

Pillow's encoder decides which blocks the JPEG kernels see; write_jpeg() hands them exactly the blocks that are hard for them, through
the public entry, as a file libjpeg-turbo decodes too.  Sequential DCT, 8-bit samples, one interleaved scan, the Annex K Huffman tables.
Also the bit-level helpers tests/test_jpeg.py re-encodes Pillow files with (_BitWriter, _huff_codes, _ZZ).
"""
import numpy as np

# zigzag index -> natural (row-major) position
_ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
       35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

# ITU-T T.81 Annex K.3 (tables K.3 to K.6): (class, id) -> (number of codes of each length 1..16, symbols in code order).
# Class 0 = DC, 1 = AC; id 0 = luminance, 1 = chrominance.  libjpeg's defaults, so any Pillow file with optimize=False carries them.
STD_HUFFMAN = {
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
             [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240,
              36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73,
              74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133,
              134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180,
              181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226,
              227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250]),
    (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240,
              21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72,
              73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131,
              132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178,
              179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218,
              226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250]),
}

# sampling -> (components, luma h factor, luma v factor); chroma is always 1x1
SAMPLINGS = {"gray": (1, 1, 1), "4:4:4": (3, 1, 1), "4:2:2": (3, 2, 1), "4:2:0": (3, 2, 2)}


def _huff_codes(counts, symbols):
    codes, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            codes[symbols[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return codes


class _BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, length):
        self.acc = (self.acc << length) | (value & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


def _code_arrays(counts, symbols):
    """symbol -> (code, length) as two 256-entry arrays; length 0 = the table has no code for the symbol"""
    code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
    for s, (c, ln) in _huff_codes(counts, symbols).items():
        code[s], length[s] = c, ln
    return code, length


def _bit_size(a):
    """number of bits of |a| (0 for 0), a < 2^15"""
    a = np.abs(a)
    n = np.zeros(a.shape, np.int64)
    for b in range(15):
        n += a >= (1 << b)
    return n


def _pack_bits(value, length):
    """token stream (value, number of bits) -> entropy-coded bytes: MSB first, padded with one-bits to a byte, 0xFF stuffed with 0x00"""
    total = int(length.sum())
    if total == 0:
        return b""
    tok = np.repeat(np.arange(len(length)), length)                          # the token each bit belongs to
    start = np.cumsum(length) - length
    shift = length[tok] - 1 - (np.arange(total) - start[tok])                 # MSB first
    bits = ((value[tok] >> shift) & 1).astype(np.uint8)
    pad = -total % 8
    if pad:
        bits = np.concatenate([bits, np.ones(pad, np.uint8)])
    by = np.packbits(bits)
    ff = np.flatnonzero(by == 0xFF)
    if len(ff):
        by = np.insert(by, ff + 1, 0)
    return by.tobytes()


def _segment(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def write_jpeg(coef, quant, width, height, sampling, orientation=1, restart_interval=0) -> bytes:
    """A baseline JPEG file that holds exactly the given quantised coefficients.

    coef      int16 blocks in natural order on the padded block grid, component after component (Y, Cb, Cr; Y alone for "gray"):
              the layout sv_oracle.jpeg_coefficients() and host.jpeg_entropy_decode() return.
    quant     one table of 64 values 1..255 in natural order per component.
    sampling  "4:4:4", "4:2:2", "4:2:0" or "gray".
    orientation      1..8; other than 1 it is written as an EXIF APP1 segment holding the one tag 0x0112.
    restart_interval MCUs per restart interval (DRI + RSTn markers), 0 for none.

    Raises ValueError for what the standard tables cannot code -- a DC difference of more than 11 bits, an AC value of more than
    10 bits -- and for arguments that do not fit each other; no value is ever clipped.
    """
    if sampling not in SAMPLINGS:
        raise ValueError(f"sampling must be one of {sorted(SAMPLINGS)}")
    ncomp, hs, vs = SAMPLINGS[sampling]
    W, H = int(width), int(height)
    if not (1 <= W <= 65535 and 1 <= H <= 65535):
        raise ValueError("width and height must be 1..65535")
    if not 1 <= orientation <= 8:
        raise ValueError("orientation must be 1..8")
    if not 0 <= restart_interval <= 65535:
        raise ValueError("restart_interval must be 0..65535")
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    samp = [(hs, vs)] + [(1, 1)] * (ncomp - 1)
    nblk = [mcux * h * mcuy * v for h, v in samp]
    coef = np.asarray(coef)
    if coef.dtype.kind not in "iu" or coef.size != 64 * sum(nblk):
        raise ValueError(f"coef must hold {64 * sum(nblk)} integers for {W}x{H} {sampling}, got {coef.size} of {coef.dtype}")
    coef = coef.astype(np.int64).reshape(-1, 64)
    quant = np.asarray(quant)
    if quant.shape != (ncomp, 64) or quant.dtype.kind not in "iu" or quant.min() < 1 or quant.max() > 255:
        raise ValueError(f"quant must be {ncomp} tables of 64 integers 1..255")

    # blocks in scan order: MCU by MCU, component by component, the luma blocks of an MCU row-major
    order, comp_of = [], []
    base = 0
    my, mx = np.mgrid[0:mcuy, 0:mcux]
    for c, (h, v) in enumerate(samp):
        bw = mcux * h
        idx = np.stack([base + (my * v + dv) * bw + mx * h + dh for dv in range(v) for dh in range(h)], -1)     # [mcuy, mcux, h*v]
        order.append(idx.reshape(mcuy * mcux, h * v))
        comp_of.append(np.full((mcuy * mcux, h * v), c))
        base += nblk[c]
    order, comp_of = np.concatenate(order, 1).ravel(), np.concatenate(comp_of, 1).ravel()
    per_mcu = len(order) // (mcuy * mcux)
    n = len(order)
    blocks = coef[order][:, _ZZ]                                             # [n, 64] in zigzag order
    interval_of = np.arange(n) // (per_mcu * restart_interval) if restart_interval else np.zeros(n, np.int64)

    # DC: difference to the previous block of the same component, predictor 0 at the start of every restart interval
    diff = np.zeros(n, np.int64)
    for c in range(ncomp):
        sel = np.flatnonzero(comp_of == c)
        dc = blocks[sel, 0]
        prev = np.concatenate([[0], dc[:-1]])
        prev[np.concatenate([[True], interval_of[sel][1:] != interval_of[sel][:-1]])] = 0
        diff[sel] = dc - prev
    dsize = _bit_size(diff)
    if dsize.max() > 11:
        b = int(np.argmax(dsize))
        raise ValueError(f"DC difference {int(diff[b])} (block {int(order[b])}) needs {int(dsize[b])} bits; the standard tables code 11")
    nzb, nzk = np.nonzero(blocks[:, 1:])
    nzk += 1
    aval = blocks[nzb, nzk]
    asize = _bit_size(aval)
    if len(asize) and asize.max() > 10:
        i = int(np.argmax(asize))
        raise ValueError(f"AC value {int(aval[i])} (block {int(order[nzb[i]])}, zigzag {int(nzk[i])}) needs {int(asize[i])} bits; the standard tables code 10")

    tabs = {k: _code_arrays(*v) for k, v in STD_HUFFMAN.items()}
    tsel = (comp_of > 0).astype(np.int64)                                    # table id: 0 for Y, 1 for Cb and Cr
    dc_code, dc_len = (np.stack([tabs[(0, t)][i] for t in (0, 1)]) for i in (0, 1))
    ac_code, ac_len = (np.stack([tabs[(1, t)][i] for t in (0, 1)]) for i in (0, 1))

    def extra(v, size):                                                      # the `size` low bits of v, or of v - 1 when v is negative
        return np.where(v > 0, v, v + (1 << size) - 1)

    # tokens (value, bits), ordered by key = (block * 65 + zigzag position) * 5 + slot: slots 0..2 are ZRLs, 3 the symbol, 4 its extra bits
    first = np.ones(len(nzb), bool)
    first[1:] = nzb[1:] != nzb[:-1]
    run = nzk - np.where(first, 0, np.concatenate([[0], nzk[:-1]])) - 1
    at = tsel[nzb]
    sym = ((run & 15) << 4) | asize
    keys = [np.arange(n) * 325 + 3, np.arange(n) * 325 + 4, (nzb * 65 + nzk) * 5 + 3, (nzb * 65 + nzk) * 5 + 4]
    vals = [dc_code[tsel, dsize], extra(diff, dsize), ac_code[at, sym], extra(aval, asize)]
    lens = [dc_len[tsel, dsize], dsize, ac_len[at, sym], asize]
    for slot in range(3):
        z = np.flatnonzero(run >= 16 * (slot + 1))
        keys.append((nzb[z] * 65 + nzk[z]) * 5 + slot)
        vals.append(ac_code[at[z], 0xF0])
        lens.append(ac_len[at[z], 0xF0])
    last = np.zeros(n, np.int64)
    last[nzb] = nzk                                                          # nzk ascends within a block: the last write wins
    eob = np.flatnonzero(last < 63)
    keys.append((eob * 65 + 64) * 5)
    vals.append(ac_code[tsel[eob], 0])
    lens.append(ac_len[tsel[eob], 0])
    keys, vals, lens = np.concatenate(keys), np.concatenate(vals), np.concatenate(lens)
    srt = np.argsort(keys, kind="stable")
    keys, vals, lens = keys[srt], vals[srt], lens[srt]

    out = bytearray(b"\xff\xd8")
    out += _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    if orientation != 1:                                                     # TIFF header, one IFD with one SHORT entry, no next IFD
        tiff = b"II\x2a\x00\x08\x00\x00\x00" + b"\x01\x00" + b"\x12\x01\x03\x00\x01\x00\x00\x00" + orientation.to_bytes(2, "little") + b"\x00\x00" + b"\x00\x00\x00\x00"
        out += _segment(0xE1, b"Exif\x00\x00" + tiff)
    for c in range(ncomp):
        out += _segment(0xDB, bytes([c]) + bytes(int(quant[c][z]) for z in _ZZ))
    out += _segment(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([ncomp])
                    + b"".join(bytes([c + 1, h << 4 | v, c]) for c, (h, v) in enumerate(samp)))
    for (tc, th), (counts, symbols) in STD_HUFFMAN.items():
        if th == 0 or ncomp == 3:
            out += _segment(0xC4, bytes([tc << 4 | th]) + bytes(counts) + bytes(symbols))
    if restart_interval:
        out += _segment(0xDD, restart_interval.to_bytes(2, "big"))
    out += _segment(0xDA, bytes([ncomp]) + b"".join(bytes([c + 1, 0x11 if c else 0x00]) for c in range(ncomp)) + b"\x00\x3f\x00")
    if restart_interval:
        tok_interval = keys // (325 * per_mcu * restart_interval)
        cuts = np.searchsorted(tok_interval, np.arange(int(tok_interval[-1]) + 2))
        for i in range(len(cuts) - 1):
            if i:
                out += bytes([0xFF, 0xD0 + (i - 1) % 8])
            out += _pack_bits(vals[cuts[i]:cuts[i + 1]], lens[cuts[i]:cuts[i + 1]])
    else:
        out += _pack_bits(vals, lens)
    return bytes(out + b"\xff\xd9")
