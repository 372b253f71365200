"""A plain numpy / Python restatement of a baseline JPEG encoder, written from the libjpeg description (jccolor.c, jcsample.c,
jcprepct.c, jccoefct.c, jfdctint.c, jcdctmgr.c, jcparam.c, jchuff.c, jcmarker.c) and from T.81, not from csrc/k17_jpeg_encode.hip or
csrc/host_jpeg.cpp.  tests/test_jpeg_encode_ref.py pins it byte for byte against Pillow (libjpeg-turbo); the GPU tests use it as the
oracle of the device half (dense coefficients, sparse records) and of the host Huffman encoder.

What it restates: JDCT_ISLOW, the Annex K Huffman tables, optimize_coding off, baseline-forced quantiser tables, JFIF 1.01 with
density 1:1, no smoothing, sampling 4:4:4 / 4:2:2 / 4:2:0 (chroma 1x1) or one gray component.

Layouts (those of the decoder, csrc/host_jpeg.cpp): coefficient blocks per component, row-major over the MCU-padded block grid, 64 values per
block in natural order; the sparse form is per block a 64-bit mask over ZIGZAG positions, the index of its first value, and the non-zero
values in zigzag order, block after block.
"""
import numpy as np

SAMPLINGS = {"gray": (1, 1, 1), "444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2)}

NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# T.81 Annex K.1, natural order
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                       + [99] * 32)

# T.81 Annex K.3: (code counts per length 1..16, symbols)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114,
            130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89,
            90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148,
            149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197,
            198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244,
            245, 246, 247, 248, 249, 250])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209,
              10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87,
              88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138,
              146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194,
              195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243,
              244, 245, 246, 247, 248, 249, 250])


def quant_tables(quality):
    """jpeg_set_quality(quality, force_baseline=TRUE): (luma, chroma), natural order"""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * scale + 50) // 100, 1, 255).astype(np.uint16) for base in (BASE_LUMA, BASE_CHROMA))


class Geometry:
    """Block grids of a W x H image: bw, bh per component over whole MCUs (the layout), own_bw, own_bh the component's own grid (jpeg_component_info
    width_in_blocks, height_in_blocks: what the encoder computes; the rest of the MCU-padded grid are dummy blocks)."""

    def __init__(self, W, H, sampling):
        self.W, self.H, self.sampling = W, H, sampling
        self.ncomp, self.hs, self.vs = SAMPLINGS[sampling]
        self.mcu_cols = -(-W // (8 * self.hs))
        self.mcu_rows = -(-H // (8 * self.vs))
        self.h = [self.hs, 1, 1][:self.ncomp]
        self.v = [self.vs, 1, 1][:self.ncomp]
        self.bw = [self.mcu_cols * h for h in self.h]
        self.bh = [self.mcu_rows * v for v in self.v]
        self.own_bw = [-(-(W * h) // (self.hs * 8)) for h in self.h]
        self.own_bh = [-(-(H * v) // (self.vs * 8)) for v in self.v]
        self.block_off = np.concatenate([[0], np.cumsum([w * h for w, h in zip(self.bw, self.bh)])]).astype(np.int64)
        self.nblocks = int(self.block_off[-1])
        self.coef_count = 64 * self.nblocks


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """one pass of jfdctint.c over the last axis of d (int64 [...,8])"""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = np.empty_like(d)
    n = 11 if first else 15
    if first:
        o[..., 0], o[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[..., 0], o[..., 4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[..., 2] = _descale(z1 + t13 * 6270, n)
    o[..., 6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[..., 7] = _descale(t4 + z1 + z3, n)
    o[..., 5] = _descale(t5 + z2 + z4, n)
    o[..., 3] = _descale(t6 + z2 + z3, n)
    o[..., 1] = _descale(t7 + z1 + z4, n)
    return o


def fdct_quantise(blocks, q):
    """blocks: samples [n,8,8] (0..255); q: 64 steps, natural order -> int16 [n,64] natural order.  The quantiser divides the FDCT's
    output (scaled by 8) by 8 q, rounding half away from zero."""
    d = blocks.astype(np.int64) - 128
    d = _fdct_pass(d, True)                                              # rows
    d = _fdct_pass(d.transpose(0, 2, 1), False).transpose(0, 2, 1)      # columns
    div = q.astype(np.int64).reshape(8, 8) * 8
    out = (np.abs(d) + (div >> 1)) // div
    return (np.sign(d) * out).astype(np.int16).reshape(-1, 64)


def component_planes(img, geo):
    """jccolor.c + jcprepct.c + jcsample.c: the component planes, each own_bw*8 x own_bh*8 samples (edges replicated)."""
    H, W = geo.H, geo.W
    planes = []
    if geo.ncomp == 1:
        full = [img.astype(np.int64)]
    else:
        b, g, r = (img[..., i].astype(np.int64) for i in range(3))
        full = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
                (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16]
    for c, p in enumerate(full):
        fh, fv = geo.hs // geo.h[c], geo.vs // geo.v[c]               # down-sampling factors of this component
        pw, ph = geo.own_bw[c] * 8, geo.own_bh[c] * 8
        # the colour rows are padded to a whole row group by repeating the last one, every row to pw * fh columns by repeating the last
        rows = -(-H // geo.vs) * geo.vs
        p = np.concatenate([p, np.repeat(p[-1:], rows - H, 0)], 0)
        p = np.concatenate([p, np.repeat(p[:, -1:], pw * fh - W, 1)], 1) if pw * fh > W else p[:, :pw * fh]
        if fh == 2 and fv == 1:
            bias = np.arange(pw) & 1                                    # 0, 1, 0, 1, ...
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        elif fh == 2 and fv == 2:
            bias = 1 + (np.arange(pw) & 1)                              # 1, 2, 1, 2, ...
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        # the down-sampled rows are padded to a whole iMCU row by repeating the last one
        p = np.concatenate([p, np.repeat(p[-1:], ph - p.shape[0], 0)], 0) if ph > p.shape[0] else p[:ph]
        planes.append(p)
    return planes


def forward(img, quality, sampling):
    """img: u8 [H,W,3] BGR or [H,W] gray -> (Geometry, int16 coefficients [coef_count] in the layout above, uint16 quant [3,64])"""
    img = np.asarray(img)
    H, W = img.shape[:2]
    geo = Geometry(W, H, sampling)
    assert (img.ndim == 2) == (geo.ncomp == 1)
    ql, qc = quant_tables(quality)
    quant = np.zeros((3, 64), np.uint16)
    coef = np.zeros((geo.nblocks, 64), np.int16)
    for c, p in enumerate(component_planes(img, geo)):
        q = ql if c == 0 else qc
        quant[c] = q
        obw, obh = geo.own_bw[c], geo.own_bh[c]
        blocks = p.reshape(obh, 8, obw, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
        grid = np.zeros((geo.bh[c], geo.bw[c], 64), np.int16)
        grid[:obh, :obw] = fdct_quantise(blocks, q).reshape(obh, obw, 64)
        # jccoefct.c: dummy blocks have zero AC and the DC of the block before them in the MCU
        h, v = geo.h[c], geo.v[c]
        for my in range(geo.mcu_rows):
            for mx in range(geo.mcu_cols):
                prev = 0
                for y in range(my * v, my * v + v):
                    for x in range(mx * h, mx * h + h):
                        if y >= obh or x >= obw:
                            grid[y, x, 0] = prev
                        prev = grid[y, x, 0]
        coef[geo.block_off[c]:geo.block_off[c + 1]] = grid.reshape(-1, 64)
    return geo, coef.reshape(-1), quant


def sparse(coef):
    """dense coefficients -> (masks u64 [nb], offsets u32 [nb], values i16 [count]): the transport form"""
    zz = coef.reshape(-1, 64)[:, NATURAL]
    nz = zz != 0
    masks = (nz.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64)
    counts = nz.sum(1)
    offsets = (np.cumsum(counts) - counts).astype(np.uint32)
    return masks, offsets, zz[nz].astype(np.int16)


def _huff_codes(table):
    counts, symbols = table
    code, k, out = 0, 0, {}
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)                                      # byte stuffing
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)               # pad with 1 bits


def _encode_block(bits, zz, pred, dc, ac):
    diff = int(zz[0]) - pred
    size = abs(diff).bit_length()
    bits.put(*dc[size])
    if size:
        bits.put((diff if diff > 0 else diff - 1) & ((1 << size) - 1), size)
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*ac[0xF0])                                         # ZRL
            run -= 16
        size = abs(v).bit_length()
        bits.put(*ac[(run << 4) | size])
        bits.put((v if v > 0 else v - 1) & ((1 << size) - 1), size)
        run = 0
    if run:
        bits.put(*ac[0x00])                                             # EOB


def header(geo, quant, restart):
    """SOI, APP0, DQT, SOF0, DHT, DRI, SOS as jcmarker.c writes them"""
    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)
    out = bytes([0xFF, 0xD8]) + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in range(2 if geo.ncomp == 3 else 1):
        out += seg(0xDB, bytes([t]) + bytes(int(quant[t][NATURAL[i]]) for i in range(64)))
    sof = bytes([8]) + geo.H.to_bytes(2, "big") + geo.W.to_bytes(2, "big") + bytes([geo.ncomp])
    for c in range(geo.ncomp):
        sof += bytes([c + 1, geo.h[c] << 4 | geo.v[c], 0 if c == 0 else 1])
    out += seg(0xC0, sof)
    tables = [(0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)][:4 if geo.ncomp == 3 else 2]
    for tc, (counts, symbols) in tables:
        out += seg(0xC4, bytes([tc]) + bytes(counts) + bytes(symbols))
    if restart:
        out += seg(0xDD, restart.to_bytes(2, "big"))
    sos = bytes([geo.ncomp])
    for c in range(geo.ncomp):
        sos += bytes([c + 1, 0x00 if c == 0 else 0x11])
    return out + seg(0xDA, sos + bytes([0, 63, 0]))


def entropy_encode(geo, coef, quant, restart=0):
    """dense coefficients -> the bytes of the file"""
    zz = coef.reshape(-1, 64)[:, NATURAL]
    dc = [_huff_codes(DC_LUMA), _huff_codes(DC_CHROMA)]
    ac = [_huff_codes(AC_LUMA), _huff_codes(AC_CHROMA)]
    out = bytearray(header(geo, quant, restart))
    bits, pred, rst = _Bits(), [0, 0, 0], 0
    for mi in range(geo.mcu_cols * geo.mcu_rows):
        if restart and mi and mi % restart == 0:
            bits.flush()
            out += bits.out + bytes([0xFF, 0xD0 + (rst & 7)])
            bits, pred, rst = _Bits(), [0, 0, 0], rst + 1
        my, mx = divmod(mi, geo.mcu_cols)
        for c in range(geo.ncomp):
            for v in range(geo.v[c]):
                for u in range(geo.h[c]):
                    bi = int(geo.block_off[c]) + (my * geo.v[c] + v) * geo.bw[c] + mx * geo.h[c] + u
                    _encode_block(bits, zz[bi], pred[c], dc[c > 0], ac[c > 0])
                    pred[c] = int(zz[bi][0])
    bits.flush()
    return bytes(out + bits.out + bytes([0xFF, 0xD9]))


def encode(img, quality=95, sampling="420", restart=0):
    geo, coef, quant = forward(img, quality, sampling)
    return entropy_encode(geo, coef, quant, restart)


# ---- shared by the encoder's test files: the case list and Pillow as the checker of record --------------------------
SIZES = [(8, 8), (16, 16), (17, 33), (33, 17), (40, 24), (1, 1), (100, 7)]          # (H, W)
QUALITIES = [1, 50, 75, 95, 100]
RESTARTS = [0, 1, 3]
CONTENTS = ["noise", "checker", "zeros", "ones", "ramp", "photo"]


def content(kind, H, W, gray=False):
    """the test inputs: u8 [H,W,3] BGR, or [H,W] when gray"""
    import os
    shape = (H, W) if gray else (H, W, 3)
    if kind == "noise":
        return np.random.RandomState(H * 1000 + W + gray).randint(0, 256, shape, dtype=np.uint8)
    if kind == "checker":
        a = (((np.arange(H)[:, None] + np.arange(W)[None, :]) & 1) * 255).astype(np.uint8)
        return a if gray else np.repeat(a[:, :, None], 3, 2)
    if kind in ("zeros", "ones"):
        return np.full(shape, 0 if kind == "zeros" else 255, np.uint8)
    if kind == "ramp":
        # a ramp leaves a block's energy in its first row and column; the faint ripple at the highest frequency puts one more value at
        # the end of the zigzag, 16 and more zeros after the last of those
        y, x = np.arange(H)[:, None], np.arange(W)[None, :]
        a = 2 * y + 3 * x + 12 * np.cos((2 * x + 1) * 7 * np.pi / 16) * np.cos((2 * y + 1) * 7 * np.pi / 16)
        a = np.clip(np.round(a), 0, 255).astype(np.uint8)
        return a if gray else np.stack([a, 255 - a, a // 2 + 60], 2)
    if kind == "photo":
        from PIL import Image
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_1.jpg")
        rgb = np.asarray(Image.open(path).convert("RGB"))
        y0, x0 = rgb.shape[0] // 2, rgb.shape[1] // 2
        crop = rgb[y0:y0 + 64, x0:x0 + 64, ::-1]
        crop = np.tile(crop, (-(-H // 64), -(-W // 64), 1))[:H, :W]
        return np.ascontiguousarray(crop[..., 1] if gray else crop)
    raise ValueError(kind)


def pillow_encode(img, quality, sampling, restart=0):
    import io
    from PIL import Image
    img = np.asarray(img)
    im = Image.fromarray(img, "L") if img.ndim == 2 else Image.fromarray(np.ascontiguousarray(img[..., ::-1]), "RGB")
    kw = {} if img.ndim == 2 else {"subsampling": {"444": 0, "422": 1, "420": 2}[sampling]}
    if restart:
        kw["restart_marker_blocks"] = restart
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=quality, optimize=False, progressive=False, **kw)
    return buf.getvalue()
