"""Inputs built for the edges of csrc/k7_preprocess_v2.hip, shared by tests/test_gpu_preprocess_v2_edges.py (GPU) and
tests/test_preprocess_v2_edges_ref.py (CPU): image builders, CLAHE tiles whose clipped total has a chosen residual, the search for
Sauvola ties, the footprint an impulse dilates to, and the bookkeeping that turns a case into its expected output
(tests/preprocess_v2_ref.py) once and keeps it.  Nothing here knows the kernels' tile sizes: the GPU module names them and
builds its case lists from them."""
from collections import namedtuple

import numpy as np

import preprocess_v2_ref as R


# ---- image builders: u8 [H,W] -----------------------------------------------------------------------------------------------
def flat(shape, v):
    return np.full(shape, v, np.uint8)


def checker(shape, lo=0, hi=255):
    yy, xx = np.indices(shape)
    return np.where((yy + xx) % 2, hi, lo).astype(np.uint8)


def stripes_h(shape, period=1, lo=0, hi=255):
    """Horizontal stripes: rows change every `period` rows."""
    yy, _ = np.indices(shape)
    return np.where((yy // period) % 2, hi, lo).astype(np.uint8)


def stripes_v(shape, period=1, lo=0, hi=255):
    """Vertical stripes: columns change every `period` columns."""
    _, xx = np.indices(shape)
    return np.where((xx // period) % 2, hi, lo).astype(np.uint8)


def two_level(shape, lo, hi, split):
    """Columns left of `split` hold lo, the others hi."""
    a = np.full(shape, hi, np.uint8)
    a[:, :split] = lo
    return a


def impulse(shape, y, x, on=255, off=0):
    a = np.full(shape, off, np.uint8)
    a[y, x] = on
    return a


def noise(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


def extreme(shape):
    """The issue's "extreme" contents: names and frames."""
    return ["flat 0", "flat 255", "checker"], np.stack([flat(shape, 0), flat(shape, 255), checker(shape)])


# ---- cases --------------------------------------------------------------------------------------------------------------------
# op: box_mean (k) | sauvola (window, k) | clahe (clip, tiles) | dilate / erode / close / open (shape, k) | gauss ()
# img: u8 [n,H,W]; names: what frame f holds; ref: "R" (the restatement) or "direct" (morph_direct, below)
Case = namedtuple("Case", "id op args img names ref")

_MORPH = {"dilate": R.dilate, "erode": R.erode, "close": R.morph_close, "open": R.morph_open}
MORPH_OPS = tuple(_MORPH)                                   # in the order of Context.MORPH_DILATE .. MORPH_OPEN


def case(id, op, args, img, names=None, ref="R"):
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        img = img[None]
    assert img.ndim == 3 and ref in ("R", "direct")
    names = list(names) if names is not None else [f"frame {f}" for f in range(len(img))]
    assert len(names) == len(img)
    return Case(id, op, tuple(args), np.ascontiguousarray(img), names, ref)


def _expected_frame(c, frame):
    if c.op == "box_mean":
        return R.box_mean(frame, *c.args)
    if c.op == "sauvola":
        return R.threshold_sauvola(frame, *c.args)
    if c.op == "clahe":
        return R.clahe(frame, *c.args)
    if c.op == "gauss":
        return R.gaussian_blur21(frame)
    el = R.structuring_element(*c.args)
    if c.ref == "direct":
        return morph_direct(frame, el, c.op)
    return _MORPH[c.op](frame, el)


_EXPECTED = {}


def expected(c):
    """u8 [n,H,W]: computed once per case id, shared by every test that asks, and never written to."""
    if c.id not in _EXPECTED:
        out = np.stack([_expected_frame(c, f) for f in c.img])
        out.setflags(write=False)
        _EXPECTED[c.id] = (c, out)
    assert _EXPECTED[c.id][0] is c, f"two cases share the id {c.id}"
    return _EXPECTED[c.id][1]


# ---- morphology: the footprint of an impulse, and the definition for elements far larger than the image -------------------------
def impulse_footprint(shape, y0, x0, el):
    """What dilating one 255 pixel at (y0, x0) on zeros must give: dst(x, y) takes src(x + j - a, y + i - a) for el[i, j] = 1, so the
    impulse reaches the pixels (y0 - (i - a), x0 - (j - a)): the element reflected through its anchor a = k // 2, clipped to the image."""
    k = el.shape[0]
    a = k // 2
    out = np.zeros(shape, np.uint8)
    for i, j in np.argwhere(el):
        y, x = y0 - (i - a), x0 - (j - a)
        if 0 <= y < shape[0] and 0 <= x < shape[1]:
            out[y, x] = 255
    return out


def morph_direct(img, el, op):
    """dilate / erode / close / open by the definition, visiting only the element rows that can land on an image row: O(H^2 W^2), for
    images of a few rows under elements of thousands (R._morph pads by k on every side and slides over the padding once per distinct
    row span, minutes at k = 4095).  tests/test_preprocess_v2_edges_ref.py holds it to R on the sizes R can afford."""
    if op == "close":
        return morph_direct(morph_direct(img, el, "dilate"), el, "erode")
    if op == "open":
        return morph_direct(morph_direct(img, el, "erode"), el, "dilate")
    fn, ident = (np.maximum, 0) if op == "dilate" else (np.minimum, 255)
    H, W = img.shape
    k = el.shape[0]
    a = k // 2
    out = np.full((H, W), ident, np.uint8)
    xs = np.arange(W)
    for i in range(max(0, a - (H - 1)), min(k, a + H)):
        ones = np.flatnonzero(el[i])
        if not ones.size:
            continue
        lo, hi = xs + (ones[0] - a), xs + (ones[-1] - a)                       # pixel x takes the columns lo[x] .. hi[x] of row y + dy
        inside = (xs[None, :] >= lo[:, None]) & (xs[None, :] <= hi[:, None])  # [x, column]
        dy = i - a
        ys = np.arange(max(0, -dy), min(H, H - dy))
        taken = np.where(inside[None], img[ys + dy][:, None, :], ident)
        out[ys] = fn(out[ys], fn.reduce(taken, axis=2).astype(np.uint8))
    return out


# ---- CLAHE: a tile whose clipped total has residual r --------------------------------------------------------------------------
def clahe_clip_limit(clip, area):
    return max(int(clip * area / 256), 1) if clip > 0 else 0


def clahe_residual_tile(th, tw, clip, r, m, a, seed):
    """-> (u8 [th,tw], r).  Value `a` takes L + r + 256 m pixels (L the clip limit), so it alone is clipped and the clipped total is
    r + 256 m; the rest goes to as few other values as can hold it with at most L pixels each, then the positions are shuffled."""
    area = th * tw
    L = clahe_clip_limit(clip, area)
    na = L + r + 256 * m
    rest = area - na
    others = -(-rest // L) if rest else 0
    assert L > 0 and rest >= 0 and others <= 255, (area, L, na)
    values = [(a + 7 * (i + 1)) % 256 for i in range(256)]                   # 7 is coprime to 256: every value once, `a` last
    assert values[255] == a and len(set(values)) == 256
    px = np.full(area, a, np.uint8)
    px[na:] = np.array(values[:others] * L, np.uint8)[:rest] if rest else []
    assert np.bincount(px, minlength=256)[a] == na and np.delete(np.bincount(px, minlength=256), a).max(initial=0) <= L
    return np.random.RandomState(seed).permutation(px).reshape(th, tw), r


def clahe_residual(tile, clip):
    """The residual CLAHE is left with on this tile, from its histogram in plain numpy."""
    hist = np.bincount(tile.ravel(), minlength=256)
    return int(np.maximum(hist - clahe_clip_limit(clip, tile.size), 0).sum()) % 256


# ---- Sauvola: 3 x 3 images whose centre pixel equals its threshold --------------------------------------------------------------
TIE_LEVELS = (0, 64, 128, 192, 255)
TIE_KS = (0.0, 0.2, 0.5)
TIE_KEEP = 32


def sauvola_ties():
    """Every 3 x 3 image over TIE_LEVELS, window 3: the centre's window is the whole image, so its sums are the image's.  Images are
    enumerated as base-5 numbers, first pixel most significant; an image is taken once per k of TIE_KS (in that order) at which
    float(centre) == threshold in the restatement's float32 sequence; the first TIE_KEEP (image, k) pairs are kept.
    -> [(u8 [3,3], k)], the same list on every call."""
    lv = np.array(TIE_LEVELS, np.int64)
    n = len(lv) ** 9
    digits = (np.arange(n)[:, None] // len(lv) ** np.arange(8, -1, -1)[None, :]) % len(lv)
    px = lv[digits]                                                           # [n, 9]
    s1, s2, centre = px.sum(1), (px * px).sum(1), px[:, 4].astype(np.float32)
    tie = np.stack([centre == R.sauvola_threshold_from_sums(s1, s2, 3, k) for k in TIE_KS], axis=1)   # [n, len(TIE_KS)]
    kept = np.argwhere(tie)[:TIE_KEEP]                                        # row-major: by image, then by k
    return [(px[i].reshape(3, 3).astype(np.uint8), TIE_KS[j]) for i, j in kept]
