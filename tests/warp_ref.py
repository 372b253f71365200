"""An independent, vectorised float64 restatement of the perspective-warp family (CPU, numpy): OpenCV's classic fixed-point
warpPerspective (INTER_LINEAR, BORDER_CONSTANT 0) and 8-bit resize INTER_LINEAR, written from the algorithm DESIGN.md section 2
describes, plus a continuous bilinear reference with a per-pixel error bound, and GEOMETRIES: the named hard cases every kernel
of the family is tested at (tests/test_warp_ref.py on the CPU, tests/test_gpu_warp_geometry.py on the GPU).

warpPerspective, as OpenCV's WarpPerspectiveInvoker computes it for a destination of S x S:
  * the destination is cut into blocks of bh = min(16, S) rows and bw = min(1024 / bh, S) columns;
  * for every destination row y and block origin x0 it evaluates, in float64, X0 = (M0*x0 + M1*y) + M2 (likewise Y0 with M3..M5
    and W0 with M6..M8); a pixel x1 columns right of the origin then uses W = W0 + M6*x1, W = 32/W (0 when W is 0),
    fX = (X0 + M0*x1)*W, fY = (Y0 + M3*x1)*W;
  * fX, fY are clamped to the int32 range and rounded half to even; the source cell is (X >> 5, Y >> 5) saturated to int16 and
    the 1/32 fractions are (X & 31, Y & 31);
  * the four taps get the 15-bit weights (32-a)(32-b)*32, a(32-b)*32, (32-a)b*32, ab*32 (they sum to 2^15); a tap outside the
    image contributes 0; the result is (sum + 2^14) >> 15 per channel.
numpy's elementwise float64 multiply and add each round once, as the no-FMA C does.

resize INTER_LINEAR on 8-bit (cv2.resize's fixed-point path with 11-bit coefficients): per destination index d,
f = float32((d + 0.5)*scale - 0.5) with scale = 1/(d_len/s_len), s = floor(f), f -= s (float32), weights
rint((1-f)*2048), rint(f*2048) in float32.  Horizontally an offset < 0 or >= s_len-1 collapses to the edge pixel with weights
(2048, 0); vertically the two source rows are clamped into the image.  The horizontal pass gives t = S[s]*w0 + S[s+1]*w1, the
vertical one ((b0*(t0 >> 4)) >> 16) + ((b1*(t1 >> 4)) >> 16) + 2) >> 2.  Resizing to the same size is a copy.

MUTATIONS name small, plausible mistakes a kernel could make in these rules; `warp`, `resize`, `cells` and `band_counts` take
mutation= to compute them, and tests/test_warp_ref.py checks that GEOMETRIES notices every one of them.
"""
from dataclasses import dataclass, field

import numpy as np

FRAC_BITS = 5
INT_MIN, INT_MAX = -2147483648.0, 2147483647.0

MUTATIONS = {
    "per_pixel_origin": "the homography evaluated afresh at every pixel instead of at the block origin plus M0*x1",
    "block_w_32": "block width 32 instead of min(1024 / min(16, S), S)",
    "half_away": "the x32 coordinate rounded half away from zero instead of half to even",
    "trunc_div": "source cell X / 32 truncated toward zero instead of the arithmetic X >> 5",
    "no_int16_sat": "the source cell not saturated to the int16 range",
    "replicate_border": "taps outside the image read the nearest edge pixel instead of 0",
    "frac_bits_4": "4 fraction bits (1/16 px) instead of 5",
    "resize_trunc": "resize weights (1-f)*2048 and f*2048 truncated instead of rounded",
}
WARP_MUTATIONS = tuple(m for m in MUTATIONS if m != "resize_trunc")


def _check_mutation(mutation):
    if mutation is not None and mutation not in MUTATIONS:
        raise ValueError(f"unknown mutation {mutation!r}")


def block_width(S, mutation=None):
    if mutation == "block_w_32":
        return min(32, S)
    return min(1024 // min(16, S), S)


def coords(Minv, S, mutation=None):
    """Destination S x S -> (sx, sy, a, b, X, Y) int64 arrays [S,S]: source cell, fractions and the rounded x32 coordinates."""
    _check_mutation(mutation)
    M = np.asarray(Minv, np.float64).reshape(9)
    fb = 4 if mutation == "frac_bits_4" else FRAC_BITS
    one = float(1 << fb)
    dy = np.arange(S, dtype=np.float64)[:, None]
    dx = np.arange(S)[None, :]
    bw = block_width(S, mutation)
    x0i = (dx // bw) * bw
    if mutation == "per_pixel_origin":
        x0i = dx
    x0, x1 = x0i.astype(np.float64), (dx - x0i).astype(np.float64)
    X0 = M[0] * x0 + M[1] * dy + M[2]
    Y0 = M[3] * x0 + M[4] * dy + M[5]
    W0 = M[6] * x0 + M[7] * dy + M[8]
    Wd = W0 + M[6] * x1
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Wr = np.where(Wd != 0, one / np.where(Wd != 0, Wd, 1.0), 0.0)
        fX = np.clip((X0 + M[0] * x1) * Wr, INT_MIN, INT_MAX)
        fY = np.clip((Y0 + M[3] * x1) * Wr, INT_MIN, INT_MAX)
    if mutation == "half_away":
        X = (np.sign(fX) * np.floor(np.abs(fX) + 0.5)).astype(np.int64)
        Y = (np.sign(fY) * np.floor(np.abs(fY) + 0.5)).astype(np.int64)
    else:
        X, Y = np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)
    X, Y = np.clip(X, -2 ** 31, 2 ** 31 - 1), np.clip(Y, -2 ** 31, 2 ** 31 - 1)
    if mutation == "trunc_div":
        sx, sy = np.fix(X / one).astype(np.int64), np.fix(Y / one).astype(np.int64)
    else:
        sx, sy = X >> fb, Y >> fb
    if mutation != "no_int16_sat":
        sx, sy = np.clip(sx, -32768, 32767), np.clip(sy, -32768, 32767)
    mask = (1 << fb) - 1
    return sx, sy, X & mask, Y & mask, X, Y


def sample(img, sx, sy, a, b, mutation=None):
    """Bilinear taps with fixed-point weights at cells (sx, sy), fractions (a, b): uint8 [..., C] (or [...] for a gray image)."""
    img = np.asarray(img, np.uint8)
    gray = img.ndim == 2
    im = img[..., None] if gray else img
    H, W = im.shape[:2]
    T = 16 if mutation == "frac_bits_4" else 32
    unit = (1 << 15) // (T * T)                      # the four weights sum to 2^15

    def tap(x, y):
        xc, yc = np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)
        v = im[yc, xc].astype(np.int64)
        if mutation != "replicate_border":
            v = v * ((x >= 0) & (x < W) & (y >= 0) & (y < H))[..., None]
        return v

    a, b = a[..., None], b[..., None]
    acc = (tap(sx, sy) * ((T - a) * (T - b) * unit) + tap(sx + 1, sy) * (a * (T - b) * unit) +
           tap(sx, sy + 1) * ((T - a) * b * unit) + tap(sx + 1, sy + 1) * (a * b * unit))
    out = ((acc + (1 << 14)) >> 15).astype(np.uint8)
    return out[..., 0] if gray else out


def warp(img, Minv, S, mutation=None):
    """cv2.warpPerspective(img, inv(Minv), (S, S)) with INTER_LINEAR / BORDER_CONSTANT 0: uint8 [S,S] or [S,S,C]."""
    sx, sy, a, b, _, _ = coords(Minv, S, mutation)
    return sample(img, sx, sy, a, b, mutation)


def resize_table(s_len, d_len, mutation=None):
    """-> (offset int64 [d_len], w0, w1 int64 [d_len]) before any edge handling."""
    scale = 1.0 / (d_len / s_len)
    f = ((np.arange(d_len, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    f = (f - s).astype(np.float32)
    rnd = np.trunc if mutation == "resize_trunc" else np.rint
    w0 = rnd((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    w1 = rnd(f * np.float32(2048)).astype(np.int64)
    return s.astype(np.int64), w0, w1


def resize(img, dsize, mutation=None):
    """cv2.resize(img, dsize=(dw, dh), interpolation=INTER_LINEAR) of a gray uint8 image."""
    _check_mutation(mutation)
    img = np.asarray(img, np.uint8)
    sh, sw = img.shape
    dw, dh = dsize
    if (sh, sw) == (dh, dw):
        return img.copy()
    xo, a0, a1 = resize_table(sw, dw, mutation)
    edge = (xo < 0) | (xo >= sw - 1)
    xo = np.where(xo < 0, 0, np.where(xo >= sw - 1, sw - 1, xo))
    a0, a1 = np.where(edge, 2048, a0), np.where(edge, 0, a1)
    x1 = np.minimum(xo + 1, sw - 1)
    yo, b0, b1 = resize_table(sh, dh, mutation)
    y0, y1 = np.clip(yo, 0, sh - 1), np.clip(yo + 1, 0, sh - 1)
    src = img.astype(np.int64)
    t0 = src[y0][:, xo] * a0 + src[y0][:, x1] * a1
    t1 = src[y1][:, xo] * a0 + src[y1][:, x1] * a1
    out = (((b0[:, None] * (t0 >> 4)) >> 16) + ((b1[:, None] * (t1 >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def bgr_to_gray(bgr):
    """cv2.cvtColor(BGR2GRAY) on 8-bit: 15-bit coefficients, rounded."""
    p = np.asarray(bgr, np.int64)
    return ((p[..., 0] * 3735 + p[..., 1] * 19235 + p[..., 2] * 9798 + 16384) >> 15).astype(np.uint8)


def extract(grid, cell_size=28, margin_ratio=0.1, mutation=None):
    """extract_cells (cv/extract.py): 81 crops of the (h/9 x w/9) cells less int(cell * margin_ratio) a side, gray, resized."""
    grid = np.asarray(grid, np.uint8)
    h, w = grid.shape[:2]
    ch, cw = h // 9, w // 9
    mh, mw = int(ch * margin_ratio), int(cw * margin_ratio)
    g = bgr_to_gray(grid) if grid.ndim == 3 else grid
    out = np.empty((81, cell_size, cell_size), np.uint8)
    for r in range(9):
        for c in range(9):
            crop = g[r * ch + mh:(r + 1) * ch - mh, c * cw + mw:(c + 1) * cw - mw]
            out[r * 9 + c] = resize(crop, (cell_size, cell_size), mutation)
    return out


def cells(frame, Minv, mutation=None):
    """The K2 path: warp a BGR frame to 450 x 450, then extract_cells' 81 gray 40 x 40 crops resized to 28 x 28."""
    return extract(warp(frame, Minv, 450, mutation), 28, 0.1, mutation)


BAND_HALF, QS = 2, 450


def band_counts(binary, Minv, mutation=None):
    """grid_quality's compute_completeness counts: pixels > 0 of the 450 x 450 warp of `binary` in the 20 bands
    (band 2i = rows around grid line i, 2i+1 = columns around it; a band is the line +-2, clipped to the image)."""
    wp = warp(binary, Minv, QS, mutation) > 0
    out = []
    for i in range(10):
        c = min(i * (QS // 9), QS - 1)
        lo, hi = max(0, c - BAND_HALF), min(QS, c + BAND_HALF + 1)
        out += [int(wp[lo:hi, :].sum()), int(wp[:, lo:hi].sum())]
    return np.array(out, np.int64)


# ---- homography: order_points, inset and an independent DLT -------------------------------------------------------------------
def order_points(pts):
    """cv/grid.py's order_points: TL = argmin(x+y), TR = argmin(y-x), BR = argmax(x+y), BL = argmax(y-x), float32 sums, first
    index on ties (numpy's argmin / argmax)."""
    p = np.asarray(pts, np.float32).reshape(4, 2)
    s, d = p[:, 0] + p[:, 1], p[:, 1] - p[:, 0]
    return p[[np.argmin(s), np.argmin(d), np.argmax(s), np.argmax(d)]]


def inset_corners(rect, inset):
    """cv/grid.py's inset toward the centroid in float32 numpy arithmetic (inset 0 leaves the corners unchanged)."""
    r = np.asarray(rect, np.float32)
    cx = np.float32(((r[0, 0] + r[1, 0]) + r[2, 0]) + r[3, 0]) / np.float32(4)
    cy = np.float32(((r[0, 1] + r[1, 1]) + r[2, 1]) + r[3, 1]) / np.float32(4)
    out = np.empty_like(r)
    for i in range(4):
        dx, dy = np.float32(cx - r[i, 0]), np.float32(cy - r[i, 1])
        dist = np.sqrt(np.float32(dx * dx + dy * dy))
        amt = np.float32(dist * np.float32(inset))
        out[i] = (r[i, 0] + (dx / dist) * amt, r[i, 1] + (dy / dist) * amt)
    return out


def square(S):
    return np.array([[0, 0], [S - 1, 0], [S - 1, S - 1], [0, S - 1]], np.float64)


def homography(corners, S, inset=0.0):
    """Source -> destination homography (float64 [3,3], H[2,2] = 1) of the ordered, inset corners onto the square
    (0,0)..(S-1,S-1), by the 8-unknown DLT solved with np.linalg.solve.  Raises ValueError when the corners order to a
    degenerate quad."""
    src = inset_corners(order_points(corners), inset).astype(np.float64)
    dst = square(S)
    A, rhs = np.zeros((8, 8)), np.zeros(8)
    for i, ((x, y), (u, v)) in enumerate(zip(src, dst)):
        A[2 * i] = [x, y, 1, 0, 0, 0, -x * u, -y * u]
        A[2 * i + 1] = [0, 0, 0, x, y, 1, -x * v, -y * v]
        rhs[2 * i], rhs[2 * i + 1] = u, v
    if len({tuple(p) for p in src}) < 4 or np.linalg.matrix_rank(A) < 8:
        raise ValueError("degenerate quad")
    return np.append(np.linalg.solve(A, rhs), 1.0).reshape(3, 3)


def project(Mat, pts):
    p = np.concatenate([np.asarray(pts, np.float64), np.ones((len(pts), 1))], 1) @ np.asarray(Mat, np.float64).T
    return p[:, :2] / p[:, 2:]


# ---- the continuous reference and its per-pixel bound ---------------------------------------------------------------------------
def warp_continuous(img, Minv, S):
    """Float64 bilinear interpolation at the exact source coordinate Minv @ (x, y, 1) of every destination pixel, taps outside
    the image 0 -> (value float64 [S,S,C], bound float64 [S,S,C]).

    The bound on |warp(img, Minv, S) - value| per pixel:
      * warp() evaluates the bilinear interpolant of the same zero-padded image at the coordinate rounded to the 1/32 lattice,
        so each axis moves by at most 1/64 px.  Integer positions lie on that lattice, so the rounded point stays in the closure
        of the exact point's cell, where the interpolant is Lipschitz with constants Dx = max(|p01-p00|, |p11-p10|) along x and
        Dy = max(|p10-p00|, |p11-p01|) along y (p.. the cell's 2 x 2 taps): the change is <= (Dx + Dy)/64.  The float64
        evaluation of the coordinate can put a point within ~1e-9 px of a rounding tie on the other side, so 1/64 is widened
        by 1e-6.
      * the 15-bit weights (32-a)(32-b)*32 / 2^15 are the exact bilinear weights at the lattice point; 1/32768 is allowed for
        their rounding all the same.
      * (sum + 2^14) >> 15 rounds the exact interpolant to the nearest integer: <= 0.5.
    bound = 0.5 + (Dx + Dy)*(1/64 + 1e-6) + 1/32768.  It does not hold where the int32 clamp or the int16 saturation moves the
    coordinate, or where W is 0 (those pixels are not a bilinear sample of the exact point)."""
    img = np.asarray(img, np.uint8)
    im = (img[..., None] if img.ndim == 2 else img).astype(np.float64)
    H, W = im.shape[:2]
    pad = np.zeros((H + 4, W + 4, im.shape[2]))
    pad[2:H + 2, 2:W + 2] = im
    M = np.asarray(Minv, np.float64).reshape(3, 3)
    ys, xs = np.mgrid[0:S, 0:S].astype(np.float64)
    w = M[2, 0] * xs + M[2, 1] * ys + M[2, 2]
    fx = (M[0, 0] * xs + M[0, 1] * ys + M[0, 2]) / w
    fy = (M[1, 0] * xs + M[1, 1] * ys + M[1, 2]) / w
    fx, fy = np.clip(fx, -3.0, W + 2.0), np.clip(fy, -3.0, H + 2.0)      # far outside: the taps are 0 either way
    x0, y0 = np.floor(fx), np.floor(fy)
    ax, by = (fx - x0)[..., None], (fy - y0)[..., None]
    xi, yi = x0.astype(np.int64) + 2, y0.astype(np.int64) + 2
    xi, yi = np.clip(xi, 0, W + 2), np.clip(yi, 0, H + 2)
    p00, p01, p10, p11 = pad[yi, xi], pad[yi, xi + 1], pad[yi + 1, xi], pad[yi + 1, xi + 1]
    val = (1 - ax) * (1 - by) * p00 + ax * (1 - by) * p01 + (1 - ax) * by * p10 + ax * by * p11
    Dx = np.maximum(np.abs(p01 - p00), np.abs(p11 - p10))
    Dy = np.maximum(np.abs(p10 - p00), np.abs(p11 - p01))
    bound = 0.5 + (Dx + Dy) * (1 / 64 + 1e-6) + 1 / 32768
    return val, bound


# ---- GEOMETRIES -------------------------------------------------------------------------------------------------------------
@dataclass
class Geometry:
    name: str
    reason: str
    H: int
    W: int
    S: int
    corners: np.ndarray = None          # float32 [4,2] (any order), or None when `minv` is given directly
    minv: np.ndarray = None             # float64 [3,3]: a hand-built destination -> source map no quad produces
    inset: float = 0.0
    exact: str = None                   # name of the closed form the warp must equal, if any
    degenerate: bool = False            # the corners order to a degenerate quad
    params: dict = field(default_factory=dict)

    @property
    def seed(self):
        return sum(ord(c) * (i + 1) for i, c in enumerate(self.name)) % 100003


def _quad(cx, cy, half_w, half_h, deg=0.0):
    t = np.deg2rad(deg)
    R = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    p = np.array([[-half_w, -half_h], [half_w, -half_h], [half_w, half_h], [-half_w, half_h]]) @ R.T
    return (p + [cx, cy]).astype(np.float32)


def _rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float32)


def _affine(a, b, c, d, e, f):
    return np.array([[a, b, c], [d, e, f], [0.0, 0.0, 1.0]])


def _tie_probe(S, mutation, bx=0.1, by=0.37):
    """An affine Minv (W = 1: the x32 scaling is exact) whose M2 is nudged ulp by ulp until `mutation`'s way of evaluating the
    block origin rounds some destination pixel's x32 coordinate differently from the block-origin rule.  The two evaluations
    are the same real number; they differ only in float64 rounding, which matters only next to a half-integer of the x32
    coordinate, so such a pixel has to be searched for."""
    for k in range(4000):
        target = (4 * S + k + 0.5) / 32.0                 # a tie of the x32 coordinate, walking along the row
        m2 = target - bx * (S - 1) - by * (S // 2)
        for step in range(-8, 9):
            M = _affine(bx, by, m2 + step * np.spacing(m2), 0.003, 1.0, 0.0)
            if (coords(M, S, mutation)[4] != coords(M, S)[4]).any():
                return M
    raise AssertionError(f"no tie probe found for {mutation}")


def _geometries():
    G = []

    def add(*a, **k):
        G.append(Geometry(*a, **k))

    # exact-answer cases: no OpenCV model needed
    add("identity", "identity corners: the warp is an exact copy of the top-left S x S", 120, 161, 100, _rect(0, 0, 99, 99), exact="identity")
    add("translate_int", "integer translation: an exact crop", 150, 203, 100, _rect(17, 9, 116, 108), exact="translate", params={"tx": 17, "ty": 9})
    add("scale_3", "integer scale 3: exactly img[::3, ::3]", 200, 250, 65, _rect(0, 0, 192, 192), exact="scale", params={"kx": 3, "ky": 3})
    add("scale_2x5", "anisotropic integer scale (2, 5): exactly img[::5, ::2]", 330, 140, 64, _rect(0, 0, 126, 315), exact="scale",
        params={"kx": 2, "ky": 5})
    add("half_pixel", "half-pixel shift: a = b = 16, every output is (p00+p01+p10+p11)*8192 + 2^14 >> 15", 90, 97, 63,
        _rect(0.5, 0.5, 62.5, 62.5), exact="half")
    # rotations, sub-pixel corners, perspective
    for deg in (10, 30, 44, 46):
        add(f"rot_{deg}", f"square rotated {deg} deg: sources cross cells diagonally", 480, 640, 450, _quad(320, 240, 170, 170, deg))
    rs = np.random.RandomState(7)
    add("subpixel", "random float corners: every coordinate sub-pixel", 300, 402, 300,
        (_rect(60, 40, 330, 260) + rs.uniform(-9, 9, (4, 2))).astype(np.float32))
    add("persp_strong", "top edge 12 % of the bottom edge: strong perspective, W varies 8x over the square", 540, 960, 450,
        np.array([[455, 60], [505, 60], [880, 500], [80, 500]], np.float32))
    add("persp_horizon", "top edge 10 %, short and tall: the vanishing line lies just above the destination square", 720, 1280, 450,
        np.array([[620, 20], [660, 20], [1100, 700], [180, 700]], np.float32))
    # scale extremes
    add("tiny_20", "a 20 px quad warped to 450: 22x upsampling, fractions walk slowly", 270, 480, 450, _quad(200, 130, 10, 10, 7))
    add("tiny_40", "a 40 px quad, slightly perspective, warped to 450", 123, 157, 450,
        np.array([[50, 40], [92, 43], [90, 81], [47, 79]], np.float32))
    add("photo_full", "the whole 3648 x 2736 frame warped to 450: 8x downsampling", 2736, 3648, 450, _rect(0, 0, 3647, 2735))
    add("frame_4k", "a 4K frame, a rotated quad at S = 1000", 2160, 3840, 1000, _quad(1900, 1100, 800, 760, 12))
    # outside the frame
    add("part_out", "one corner outside the frame: the tap-by-tap border path", 270, 480, 450,
        np.array([[-40, 30], [400, 20], [420, 250], [20, 260]], np.float32))
    add("mostly_out", "three corners outside: most samples are 0 or straddle the edge", 270, 480, 450,
        np.array([[-300, -200], [150, -180], [160, 120], [-280, 100]], np.float32))
    add("wholly_out", "the quad lies entirely outside the frame: the warp is all 0", 270, 480, 64, _rect(600, 400, 900, 700))
    add("huge_out", "corners beyond +-40000 px: x32 coordinates overflow int16 cells and saturate", 270, 480, 450,
        np.array([[-45000, -41000], [52000, -43000], [48000, 47000], [-44000, 46000]], np.float32))
    add("wide_sat", "a 40000 px wide strip: cells past 32767 saturate onto column 32767, which is inside the image", 4, 40000, 64,
        _rect(33000, 0, 39500, 3))
    # edges on the last column / row
    add("edge_exact", "the square maps exactly onto columns 0..W-1 and rows 0..H-1: taps at W-1, H-1 with zero weight beyond",
        65, 65, 65, _rect(0, 0, 64, 64), exact="identity")
    add("edge_half", "the last column/row sample half a pixel past W-1 / H-1: the inside test against the tap-by-tap path", 60, 77, 64,
        _rect(12.5, 2.5, 76.5, 59.5))
    add("edge_scale", "2x upsampling onto the last column and row: fractions 0 and 16 at W-1 and H-1", 33, 37, 65, _rect(4, 1, 36, 32))
    # frame shapes
    add("odd_frame", "odd frame W % 4 = 3, rotated quad", 271, 483, 300, _quad(240, 135, 110, 100, 21))
    add("frame_16", "a 16 x 16 frame warped to 17", 16, 16, 17, _rect(1.25, 0.75, 14.5, 15.25))
    # every block-width regime: bw = S (S <= 64), several blocks and a last partial block
    sizes = (9, 16, 17, 63, 64, 65, 300, 450, 1000)
    for S in sizes:
        add(f"S_{S}", f"S = {S}: block width {block_width(S)}, {-(-S // block_width(S))} block(s) per row", 360, 500, S,
            np.array([[70, 52], [430, 38], [452, 330], [58, 316]], np.float32))
    add("inset_005", "inset 0.05 toward the centroid (float32 arithmetic)", 300, 400, 300,
        np.array([[40, 30], [360, 45], [350, 280], [30, 265]], np.float32), inset=0.05)
    # order_points ties
    add("tie_order", "ties in x+y and in y-x: only numpy's first-index rule orders this to a proper quad", 160, 160, 64,
        np.array([[0, 40], [40, 0], [100, 60], [30, 110]], np.float32))
    add("diamond", "an exact diamond orders to TL == TR: degenerate, the identity minv", 160, 160, 64,
        np.array([[50, 0], [100, 50], [50, 100], [0, 50]], np.float32), degenerate=True)
    # hand-built maps no convex quad produces
    add("w_zero", "W0 + M6*x1 is exactly 0 at dx = 16: W := 0, so the sample reads source pixel (0, 0); W < 0 past it", 40, 50, 64,
        minv=np.array([[1.0, 0.0, 3.0], [0.0, 1.0, 2.0], [-1.0 / 16, 0.0, 1.0]]))
    add("tie_half", "x32 coordinates exactly k + 0.5 (a 1/64 px shift): half-even and half-away rounding differ", 80, 90, 64,
        minv=_affine(1.0, 0.0, 1.0 / 64, 0.0, 1.0, 3.0 / 64))
    add("tie_origin", "an M2 at which the block-origin sum and the per-pixel sum round a x32 coordinate differently", 120, 200, 64,
        minv=_tie_probe(64, "per_pixel_origin"))
    add("tie_block32", "an M2 at which origins every 32 instead of 64 columns round a x32 coordinate differently", 120, 200, 64,
        minv=_tie_probe(64, "block_w_32", bx=0.3, by=0.11))
    return G


GEOMETRIES = _geometries()
BY_NAME = {g.name: g for g in GEOMETRIES}


def frame(g, channels=3, smooth=False):
    """The seeded source image of geometry g: uint8 noise (every tap matters), or a smooth image for the continuous bound."""
    rs = np.random.RandomState(g.seed)
    shape = (g.H, g.W, channels) if channels > 1 else (g.H, g.W)
    if not smooth:
        return rs.randint(0, 256, shape, dtype=np.uint8)
    y, x = np.arange(g.H, dtype=np.float32)[:, None], np.arange(g.W, dtype=np.float32)[None, :]
    out = np.empty((g.H, g.W, channels), np.uint8)
    for c, ph in enumerate(rs.uniform(0, 6.3, channels).astype(np.float32)):
        v = 127.5 + 60 * np.sin(x / 7 + ph) * np.cos(y / 11 + ph) + 50 * (np.sin(x / 23) * np.cos(y / 23) + np.cos(x / 23) * np.sin(y / 23))
        out[..., c] = np.clip(np.rint(v), 0, 255)
    return out if channels > 1 else out[..., 0]


def closed_form(g, img):
    """The exact answer of an `exact` geometry, computed without any warp model."""
    S = g.S
    if g.exact == "identity":
        return img[:S, :S]
    if g.exact == "translate":
        return img[g.params["ty"]:g.params["ty"] + S, g.params["tx"]:g.params["tx"] + S]
    if g.exact == "scale":
        return img[::g.params["ky"], ::g.params["kx"]][:S, :S]
    if g.exact == "half":
        p = img.astype(np.int64)
        return (((p[:S, :S] + p[:S, 1:S + 1] + p[1:S + 1, :S] + p[1:S + 1, 1:S + 1]) * 8192 + 16384) >> 15).astype(np.uint8)
    raise ValueError(g.exact)
