"""Independent restatement of the component filter (sv_component_filter_u8 / sv_component_filter_bits) in numpy + scipy.ndimage, written
from the definition alone, and the inputs its tests use.  Imports nothing from the product.

The filter: with min_area = min_area_ratio * (float(H) * float(W)), every 8-connected component of foreground (pixel != 0) whose pixel
bounding box x0..x1, y0..y1 (inclusive) has float(x1 - x0) * float(y1 - y0) < min_area is erased; every other pixel is unchanged.
"""
import numpy as np
from scipy import ndimage

from despeckle_ref import noise, rectangle_outline, specks, spiral  # noqa: F401  (builders, re-exported)

_EIGHT = np.ones((3, 3), bool)


def component_filter(img, min_area_ratio):
    """img [H,W] (any dtype, foreground = non-zero) -> a copy with the components under the floor set to zero."""
    img = np.asarray(img)
    H, W = img.shape
    min_area = np.float64(min_area_ratio) * (np.float64(H) * np.float64(W))
    lab, _ = ndimage.label(img != 0, structure=_EIGHT)
    erase = np.zeros(lab.max() + 1, bool)
    for i, sl in enumerate(ndimage.find_objects(lab), 1):
        dy = np.float64(sl[0].stop - 1 - sl[0].start)
        dx = np.float64(sl[1].stop - 1 - sl[1].start)
        erase[i] = dx * dy < min_area
    out = img.copy()
    out[erase[lab]] = 0
    return out


def count_components(img):
    return int(ndimage.label(np.asarray(img) != 0, structure=_EIGHT)[1])


def pack_bits(img):
    """bool/u8 [..., H, W] with W % 32 == 0 -> int32 [..., H, W // 32], LSB = leftmost."""
    b = np.packbits(np.asarray(img) != 0, axis=-1, bitorder="little")
    return np.ascontiguousarray(b).view(np.int32)


def unpack_bits(bits, W):
    b = np.ascontiguousarray(bits).view(np.uint8)
    return np.unpackbits(b, axis=-1, bitorder="little")[..., :W].astype(bool)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------

def outline(H, W, top, left, dy, dx):
    """A 1-px rectangle outline whose bounding box differences are exactly (dy, dx)."""
    return rectangle_outline(H, W, top, top + dy, left, left + dx, thick=1)


def isolated(H, W):
    img = np.zeros((H, W), bool)
    img[::2, ::2] = True
    return img


def lattice(H, W):
    y, x = np.mgrid[:H, :W]
    return (x + y) % 2 == 0


def comb(H, W, joined="last"):
    """Vertical teeth in every second column, joined by one full row: the last (labels merge late) or the first (early)."""
    img = np.zeros((H, W), bool)
    img[:, ::2] = True
    img[:, -1] = False
    if joined == "last":
        img[-1, :-1] = True
        img[0] = False
    else:
        img[0, :-1] = True
        img[-1] = False
    return img


def frame_spiral(H, W, gap=1):
    """A 1-px path with `gap` background pixels between its turns, wound inwards until the frame is full: one long chain."""
    img = np.zeros((H, W), bool)
    top, left, bottom, right = 0, 0, H - 1, W - 1
    step = gap + 1
    first = True
    while top <= bottom and left <= right:
        img[top, (left if first else max(left - step, 0)):right + 1] = True
        img[top:bottom + 1, right] = True
        if bottom - top < step or right - left < step:
            break
        img[bottom, left:right + 1] = True
        img[top + step:bottom + 1, left] = True
        top, left, bottom, right = top + step, left + step, bottom - step, right - step
        first = False
    return img


def rings(H, W):
    """A large ring (kept at ratio 0.1) with a small blob in its hole (erased), next to a small ring with a blob in it (both erased)."""
    img = rectangle_outline(H, W, 10, H - 20, 10, W // 2 + 30, thick=2)
    img[H // 2:H // 2 + 4, W // 4:W // 4 + 5] = True
    x = W // 2 + 60
    img |= rectangle_outline(H, W, 40, 70, x, x + 40, thick=2)
    img[52:56, x + 15:x + 20] = True
    return img


def threshold_frames(H, W, ratio):
    """-> (frames bool [3,H,W], kept (dy, dx), under (dy, dx)).  Frame 0: a 1-px outline whose box product dy * dx equals the floor
    ratio * H * W exactly (kept).  Frame 1: one with (dy - 1) * (dx + 1), a little under the floor (erased).  Frame 2: both 1-px-high and
    1-px-wide lines, whose products are 0 (erased)."""
    floor = ratio * (float(H) * float(W))
    assert floor == int(floor), "choose a ratio with a whole-number floor"
    floor = int(floor)
    dy = next(d for d in range(int(floor ** 0.5), 1, -1) if floor % d == 0)
    kept, under = (dy, floor // dy), (dy - 1, floor // dy + 1)
    assert kept[0] * kept[1] == floor and under[0] * under[1] < floor and under[1] + 3 <= W and dy + 3 <= H
    lines = np.zeros((H, W), bool)
    lines[H - 1, :] = True
    lines[:H - 2, 0] = True
    return np.stack([outline(H, W, 1, 1, *kept), outline(H, W, 2, 1, *under), lines]), kept, under


def serpentine(H, W, seed):
    """(70, 8192)-style: a 1-px path that runs the whole width, turns at the ends, and fills every eighth row; specks between."""
    img = np.zeros((H, W), bool)
    rows = list(range(1, H - 1, 8))
    for i, y in enumerate(rows):
        img[y, 1:W - 1] = True
        if i + 1 < len(rows):
            x = W - 2 if i % 2 == 0 else 1
            img[y:rows[i + 1] + 1, x] = True
    return img | (specks(H, W, seed, per_tile=1.5) & ~ndimage.binary_dilation(img, structure=_EIGHT, iterations=2))
