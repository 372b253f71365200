"""The contract of K23 (sv_synth_cells_u8, include/sudoku_vision_hip.h): a numpy restatement of phase A (every background kind, grain,
artefacts, smudge, the glyph blend) and of the ops phase B adds to K22's.  Written from the header's text with plain array expressions
and no helper shared with the product; what K22 already restates (augment_ref.py, grid_v2_ref.py, warp_ref.py) is used from there.

cv2 is not available, so for the cv2 calls parity with OpenCV itself is unpinned; the numpy and Pillow arithmetic is the reference's."""
import math

import numpy as np

import augment_ref as ar
import grid_v2_ref
import warp_ref

F = np.float32
GLYPH_SIDE, BG_SLOT = 32, 255
PLAIN, TEXTURED, GRADIENT, NOISY, KEEP = range(5)
AFFINE_CONST, PERSPECTIVE_CONST, SCALE_PAD, GAUSS_BLUR, ERODE, DILATE = range(32, 38)
# 96 bytes: 18 int32, then double bg_d[3]
CELL_DTYPE = np.dtype([("bg_kind", "<i4"), ("bg_value", "<i4"), ("bg_salt", "<i4"), ("grad_dir", "<i4"), ("grain_stride", "<i4"), ("grain_d", "<u4", (2,)),
                       ("art_edges", "<i4"), ("art_width", "<i4"), ("art_dark", "<i4"), ("smudge", "<i4", (4,)), ("glyph_slot", "<i4"), ("glyph_x", "<i4"),
                       ("glyph_y", "<i4"), ("glyph_ink", "<i4"), ("bg_d", "<f8", (3,))])
S = ar.step


def cell(bg_kind=PLAIN, bg_value=255, bg_salt=0, grad_dir=0, grain=None, art=None, smudge=None, glyph=None, bg_d=()):
    """One cell record.  grain = (stride, [d per grain row]); art = (edge bits, width, darkness); smudge = (x, y, side, darkness);
    glyph = (slot, x, y, ink)."""
    c = np.zeros((), CELL_DTYPE)
    c["bg_kind"], c["bg_value"], c["grad_dir"], c["glyph_slot"] = bg_kind, bg_value, grad_dir, -1
    c["bg_salt"] = np.uint32(bg_salt & 0xffffffff).astype(np.int32)
    c["bg_d"][:len(bg_d)] = bg_d
    if grain is not None:
        c["grain_stride"] = grain[0]
        c["grain_d"] = pack_grain(grain[1])
    if art is not None:
        c["art_edges"], c["art_width"], c["art_dark"] = art
    if smudge is not None:
        c["smudge"] = smudge
    if glyph is not None:
        c["glyph_slot"], c["glyph_x"], c["glyph_y"], c["glyph_ink"] = glyph
    return c


def pack_grain(ds):
    """d of the k-th grain row in bits 2k, 2k+1 of the 64 bits (lo, hi)."""
    v = 0
    for k, d in enumerate(ds):
        v |= (int(d) & 3) << (2 * k)
    return np.array([v & 0xffffffff, v >> 32], np.uint32)


def atlas_of(masks):
    atlas, dims = np.zeros((len(masks), GLYPH_SIDE, GLYPH_SIDE), np.uint8), np.zeros((len(masks), 2), np.int32)
    for k, m in enumerate(masks):
        atlas[k, :m.shape[0], :m.shape[1]] = m
        dims[k] = (m.shape[1], m.shape[0])
    return atlas, dims


def clip_trunc(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def linspace_terms(strength, size):
    """numpy's own (start, step, stop) of np.linspace(-strength, strength, size)."""
    _, step = np.linspace(-strength, strength, size, retstep=True)
    return -strength, float(step), strength


# ---- phase A ---------------------------------------------------------------------------------------------------------------
def background_values(c, size, seed=0, index=0):
    """The float64 values before the clip and the truncation of a textured / noisy background."""
    words = ar.field_words(seed, index, BG_SLOT, int(c["bg_salt"]) & 0xffffffff, size, size)
    return float(c["bg_value"]) + float(c["bg_d"][0]) * ar.normal(words[..., 0], words[..., 1])


def background(c, size, seed=0, index=0, prev=None):
    kind, base = int(c["bg_kind"]), int(c["bg_value"])
    if kind == KEEP:
        return np.array(prev, np.uint8)
    if kind in (TEXTURED, NOISY):
        img = clip_trunc(background_values(c, size, seed, index))
        stride = int(c["grain_stride"])
        if kind == TEXTURED and 2 <= stride <= 4:
            bits = int(c["grain_d"][0]) | int(c["grain_d"][1]) << 32
            for k, y in enumerate(range(0, size, stride)):
                img[y] = np.maximum(img[y].astype(np.int64) - ((bits >> (2 * k)) & 3), 0)
        return img
    if kind == GRADIENT:
        d = [float(v) for v in c["bg_d"]]
        if int(c["grad_dir"]) in (0, 1):
            t = np.arange(size, dtype=np.float64) * d[1] + d[0]
            t[-1] = d[2]
            t = t[None, :] if int(c["grad_dir"]) == 0 else t[:, None]
            return clip_trunc(np.full((size, size), float(base)) + t)
        y, x = np.mgrid[0:size, 0:size]
        ctr = size // 2
        dist = np.sqrt(((x - ctr) ** 2 + (y - ctr) ** 2).astype(np.float64))
        return clip_trunc(float(base) - (dist / (size / 2)) * d[0])
    return np.full((size, size), base, np.uint8)


def artefacts(img, edges, width, dark):
    out = img.copy()
    if edges & 1:
        out[:width] = np.minimum(out[:width], dark)
    if edges & 2:
        out[-width:] = np.minimum(out[-width:], dark)
    if edges & 4:
        out[:, :width] = np.minimum(out[:, :width], dark)
    if edges & 8:
        out[:, -width:] = np.minimum(out[:, -width:], dark)
    return out


def smudge(img, x, y, side, dark):
    out = img.copy()
    out[y:y + side, x:x + side] = np.minimum(out[y:y + side, x:x + side], dark)
    return out


def digit_layer(size, mask, gx, gy, ink):
    """Pillow's ink over a white canvas through the coverage mask pasted at (gx, gy), clipped to the cell: u8 [size, size]."""
    m = np.zeros((size, size), np.int64)
    h, w = mask.shape
    y0, y1, x0, x1 = max(gy, 0), min(gy + h, size), max(gx, 0), min(gx + w, size)
    if y1 > y0 and x1 > x0:
        m[y0:y1, x0:x1] = mask[y0 - gy:y1 - gy, x0 - gx:x1 - gx]
    t = ink * m + 255 * (255 - m) + 128
    return ((t + (t >> 8)) >> 8).astype(np.uint8)


def multiply_blend(bg, digit):
    return (bg.astype(F) * digit.astype(F) / F(255)).astype(np.uint8)


def base_image(c, size, atlas=None, seed=0, index=0, prev=None):
    img = background(c, size, seed, index, prev)
    if int(c["art_edges"]):
        img = artefacts(img, int(c["art_edges"]), int(c["art_width"]), int(c["art_dark"]))
    if int(c["smudge"][2]):
        img = smudge(img, *[int(v) for v in c["smudge"]])
    slot = int(c["glyph_slot"])
    if slot >= 0:
        a, dims = atlas
        w, h = int(dims[slot][0]), int(dims[slot][1])
        img = multiply_blend(img, digit_layer(size, a[slot, :h, :w], int(c["glyph_x"]), int(c["glyph_y"]), int(c["glyph_ink"])))
    return img


# ---- phase B: the new ops ----------------------------------------------------------------------------------------------------
def sample_const(img, X, Y, border):
    """cv2's bilinear tap sum at the 1/32-pixel positions X, Y, BORDER_CONSTANT: a tap outside the image reads `border`."""
    if grid_v2_ref._TAB is None:
        grid_v2_ref._TAB = grid_v2_ref._bilinear_table()
    H, W = img.shape
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    w = grid_v2_ref._TAB[Y & 31, X & 31]
    acc = np.zeros(X.shape, np.int64)
    for t, (oy, ox) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        ty, tx = sy + oy, sx + ox
        inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        acc += np.where(inside, img[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)].astype(np.int64), int(border)) * w[..., t]
    return ((acc + 16384) >> 15).astype(np.uint8)


def warp_affine_const(img, M, border):
    H, W = img.shape
    return grid_v2_ref.warp_affine(img, np.asarray(M, np.float64).reshape(2, 3), (W, H), border)


def warp_perspective_const(img, M, border):
    H, W = img.shape
    X, Y = ar.perspective_coords(ar.invert3(M), H, W)
    return sample_const(img, X, Y, border)


def scale_pad(img, new_w, new_h, crop, pad):
    H, W = img.shape
    scaled = warp_ref.resize(img, (new_w, new_h))
    if crop:
        y0, x0 = (new_h - H) // 2, (new_w - W) // 2
        return scaled[y0:y0 + H, x0:x0 + W].copy()
    out = np.full((H, W), pad, np.uint8)
    y0, x0 = (H - new_h) // 2, (W - new_w) // 2
    out[y0:y0 + new_h, x0:x0 + new_w] = scaled
    return out


def gaussian_taps_q8(k, sigma):
    """-> [t0, t1, t2]: Q8.8 taps by distance, t0 + 2 t1 + 2 t2 = 256."""
    r = k // 2
    v = [math.exp(-(j * j) / (2.0 * sigma * sigma)) for j in range(r + 1)]
    total = v[0] + sum(2.0 * x for x in v[1:])
    t = [0, 0, 0]
    for j in range(1, r + 1):
        t[j] = int(np.rint(v[j] / total * 256.0))
    t[0] = 256 - 2 * t[1] - 2 * t[2]
    return t


def gauss_blur(img, k, taps):
    r = k // 2
    full = [taps[abs(j)] for j in range(-r, r + 1)]
    H, W = img.shape
    p = np.pad(img.astype(np.int64), r, mode="reflect")
    rows = sum(t * p[:, j:j + W] for j, t in enumerate(full))
    acc = sum(t * rows[j:j + H] for j, t in enumerate(full))
    return np.minimum((acc + 32768) >> 16, 255).astype(np.uint8)


def morph(img, dilate):
    fill = 0 if dilate else 255
    p = np.pad(img, ((1, 0), (1, 0)), constant_values=fill)
    stack = np.stack([p[1:, 1:], p[:-1, 1:], p[1:, :-1], p[:-1, :-1]])
    return stack.max(0) if dilate else stack.min(0)


def apply_step(img, s, seed=0, index=0, slot=0):
    op, i, d = int(s["op"]), [int(v) for v in s["i"]], s["d"]
    if op == AFFINE_CONST:
        return warp_affine_const(img, d[:6], i[0])
    if op == PERSPECTIVE_CONST:
        return warp_perspective_const(img, d, i[0])
    if op == SCALE_PAD:
        return scale_pad(img, i[0], i[1], i[2], i[3])
    if op == GAUSS_BLUR:
        return gauss_blur(img, i[0], i[1:4])
    if op in (ERODE, DILATE):
        return morph(img, op == DILATE)
    return ar.apply_step(img, s, seed, index, slot)


def run_job(cells, steps, n_steps, size, atlas=None, seed=0, index_base=0, prev=None):
    """sv_synth_cells_u8 -> u8 [n_out, size, size].  prev: what the output buffer holds before the call (KEEP cells)."""
    out = np.empty((len(cells), size, size), np.uint8)
    for o in range(len(cells)):
        img = base_image(cells[o], size, atlas, seed, index_base + o, None if prev is None else prev[o])
        for slot in range(min(max(int(n_steps[o]), 0), ar.MAX_STEPS)):
            img = apply_step(img, steps[o, slot], seed, index_base + o, slot)
        out[o] = img
    return out


def cells_array(cs):
    a = np.zeros(len(cs), CELL_DTYPE)
    for k, c in enumerate(cs):
        a[k] = c
    return a


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def sample_mask(h, w, seed=0):
    """A coverage mask like a glyph's: a ring of full coverage with soft edges, values 0 and 255 included."""
    y, x = np.mgrid[0:h, 0:w]
    r = np.hypot((x - (w - 1) / 2) / (w / 2), (y - (h - 1) / 2) / (h / 2))
    m = np.clip((1 - np.abs(r - 0.7) / 0.25) * 400, 0, 255)
    m[0, 0], m[-1, -1] = 255, 0
    rs = np.random.RandomState(seed)
    return np.clip(m + (m > 0) * (m < 255) * rs.randint(-20, 21, (h, w)), 0, 255).astype(np.uint8)
