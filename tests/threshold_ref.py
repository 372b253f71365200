"""An independent, vectorised restatement of K1 (CPU, numpy): the gray conversion, the 8-bit GaussianBlur and the GAUSSIAN_C
adaptiveThreshold that cv/preprocess.py's preprocess_for_grid_detection chains, written from OpenCV's algorithms (not from
oracle/sv_oracle.c), plus MUTATIONS, seeded tie-dense input generators and CASES: the named inputs both
tests/test_threshold_ref.py (CPU) and tests/test_gpu_threshold_geometry.py (GPU) use.  Every array function works on [..., H, W].

Rules:
  * BGR2GRAY on 8-bit: (3735*B + 19235*G + 9798*R + 2^14) >> 15, in integers.
  * GaussianBlur(ksize, 0) on 8-bit, ksize 1/3/5/7: the fixed small kernels in 8.8 fixed point (1; 64 128 64;
    16 64 96 64 16; 8 28 56 72 56 28 8: each sums to 256), horizontal pass exact, vertical pass (v + 2^15) >> 16.  Border
    BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba), reflected as often as the kernel needs (an image narrower than the radius
    reflects more than once; a one-pixel axis repeats its pixel).  ksize 1 is a copy.
  * getGaussianKernel(n, 0, CV_32F): n <= 7 the fixed table (the small kernels / 256, dyadic).  Larger n: OpenCV's bit-exact
    double path: sigma = n*0.15 + 0.35 rounded once (the fused form of 0.3*((n-1)/2 - 1) + 0.8), scale = -0.125/sigma^2,
    t_i = exp((x*x)*scale) for the doubled offsets x = 1-n, 3-n, .., sum = 2*sum(t_i) + 1, taps t_i/sum (centre 1/sum), each
    tap then converted to float.  OpenCV evaluates exp in software double; this file uses libm's exp.  The two may differ in the
    last bit of a double, which moves a float tap only if it sits within 2^-29 relative of a float rounding tie; the taps are
    compared with the C oracle bit for bit.
  * adaptiveThreshold(maxval 255, GAUSSIAN_C, type, block, C): the u8 image converted to f32, a separable f32 filter with the
    taps above and BORDER_REPLICATE, in FilterEngine's operation order with fused multiply-adds:
      - row pass, n <= 5 (SymmRowSmall): s = x_c*k_c, then s = fma(x_{c-j} + x_{c+j}, k_{c+j}, s) for j = 1..r;
      - row pass, n > 5: s = x_{-r}*k_0, then s = fma(x_j, k_j, s) from left to right;
      - column pass: s = centre*k_c, then s = fma(below_j + above_j, k_{c+j}, s) for j = 1..r (outward);
      - the mean is rint(s) (half to even), saturated to u8;
      - idelta = floor(C) for THRESH_BINARY_INV, ceil(C) for THRESH_BINARY; the lookup-table compare of d = src - mean is
        d <= -idelta (INV) or d > -idelta (BINARY).
    Every f32 operation rounds once to nearest even: products of two floats are exact in float64, and fma_f32 adds them exactly
    (TwoSum), rounds the float64 sum to odd and then to float, which is one correct rounding (the column pass can need ~69 bits,
    which a float64 fma rounded to f32 does not keep).
  * preprocess_for_grid_detection: gray -> blur(5) -> adaptive_threshold(11, 2, INV).

Parity caveat (recorded in DESIGN.md section 2, pinned here by the one_row / one_col cases): OpenCV's GaussianBlur is believed
to shrink the kernel to one tap along an axis of length 1 when the border is not CONSTANT, which would make the mean of a
one-row or one-column image the plain 1-D pass.  That rule could not be confirmed from a source here, so this file, the oracle
and the kernels all run the full 2-D filter (with REPLICATE the extra pass multiplies by the tap sum, one ulp from 1); for
ksize <= 7 the two agree exactly, for larger blocks they can differ only at a mean within ~1e-5 of a .5 tie.
"""
from dataclasses import dataclass, field
import functools
from fractions import Fraction
import math
import os

import numpy as np

MUTATIONS = {
    "gray_14bit": "gray with the 14-bit coefficients 1868/9617/4899 and + 2^13 >> 14",
    "gray_no_round": "gray without its 2^14 rounding term",
    "blur_reflect": "blur border BORDER_REFLECT (edge pixel repeated) instead of REFLECT_101",
    "blur_reflect_once": "blur border reflected only once, then clamped",
    "blur_no_round": "blur vertical pass >> 16 without the 2^15 rounding",
    "mean_reflect101": "the f32 mean with BORDER_REFLECT_101 instead of REPLICATE",
    "row_centre_first": "the row pass of blocks > 5 centre-first with symmetric pairs (SymmRowSmall) instead of left to right",
    "col_left_to_right": "the column pass top to bottom (s = x_-r*k_0, fma downward) instead of centre then pairs outward",
    "no_fma": "every multiply-add of the f32 mean rounded twice (multiply, then add)",
    "round_half_away": "the mean rounded half away from zero instead of half to even",
    "c_floor_ceil_swapped": "idelta = ceil(C) for INV and floor(C) for BINARY",
    "lt_not_le": "the compare strictness flipped: d < -idelta (INV), d >= -idelta (BINARY)",
}
ORDER_MUTATIONS = ("no_fma", "row_centre_first", "col_left_to_right")
SMALL_KERNELS = {1: (256,), 3: (64, 128, 64), 5: (16, 64, 96, 64, 16), 7: (8, 28, 56, 72, 56, 28, 8)}


def _check(mutation):
    if mutation is not None and mutation not in MUTATIONS:
        raise ValueError(f"unknown mutation {mutation!r}")


# ---- border index maps ---------------------------------------------------------------------------------------------------------
def reflect101(p, n):
    """BORDER_REFLECT_101 of positions p (any integers) into [0, n): the closed form of reflecting until inside."""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    q = np.mod(p, 2 * n - 2)
    return np.where(q < n, q, 2 * n - 2 - q)


def _reflect(p, n):                       # BORDER_REFLECT: fedcba|abcdef|fedcba
    q = np.mod(np.asarray(p, np.int64), 2 * n)
    return np.where(q < n, q, 2 * n - 1 - q)


def _reflect_once(p, n):
    p = np.asarray(p, np.int64)
    q = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))
    return np.clip(q, 0, n - 1)


# ---- gray and blur ---------------------------------------------------------------------------------------------------------------
def gray(bgr, mutation=None):
    _check(mutation)
    p = np.asarray(bgr, np.int64)
    b, g, r = p[..., 0], p[..., 1], p[..., 2]
    if mutation == "gray_14bit":
        return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)
    rnd = 0 if mutation == "gray_no_round" else 16384
    return ((3735 * b + 19235 * g + 9798 * r + rnd) >> 15).astype(np.uint8)


def blur(img, ksize=5, mutation=None):
    _check(mutation)
    img = np.asarray(img, np.uint8)
    if ksize not in SMALL_KERNELS:
        raise ValueError(ksize)
    if ksize == 1:
        return img.copy()
    H, W = img.shape[-2:]
    k, r = SMALL_KERNELS[ksize], ksize // 2
    idx = {"blur_reflect": _reflect, "blur_reflect_once": _reflect_once}.get(mutation, reflect101)
    src = img.astype(np.int64)
    xs, ys = np.arange(W), np.arange(H)
    tmp = sum(kk * src[..., idx(xs + i - r, W)] for i, kk in enumerate(k))
    v = sum(kk * tmp[..., idx(ys + i - r, H), :] for i, kk in enumerate(k))
    rnd = 0 if mutation == "blur_no_round" else 32768
    return ((v + rnd) >> 16).astype(np.uint8)


# ---- Gaussian taps -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _taps(n, fused_sigma=True):
    if n in SMALL_KERNELS:
        return tuple(np.float32(v / 256) for v in SMALL_KERNELS[n])
    if fused_sigma:
        sigma = float(Fraction(n) * Fraction(0.15) + Fraction(0.35))    # exact, then one rounding to nearest even
    else:
        sigma = ((n - 1) * 0.5 - 1) * 0.3 + 0.8
    scale = -0.125 / (sigma * sigma)
    vals = [math.exp(float(x * x) * scale) for x in range(1 - n, 0, 2)]
    s = 0.0
    for t in vals:
        s += t
    s = s * 2.0 + 1.0
    mul = 1.0 / s
    half = [np.float32(t * mul) for t in vals]
    return tuple(half + [np.float32(mul)] + half[::-1])


def gaussian_kernel_f32(n, fused_sigma=True):
    """getGaussianKernel(n, 0, CV_32F) as float32 [n] (fused_sigma=False: sigma from the unfused textbook expression)."""
    if n < 1 or n % 2 == 0:
        raise ValueError(n)
    return np.array(_taps(n, fused_sigma), np.float32)


# ---- exact f32 arithmetic ---------------------------------------------------------------------------------------------------
def fma_f32(a, b, c):
    """fmaf(a, b, c) for float32 arrays with one rounding to nearest even: exact product in float64, TwoSum, round to odd,
    then float64 -> float32."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    nudge = (err != 0) & even
    s = np.where(nudge, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def mul_f32(a, b):
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)).astype(np.float32)


def add_f32(a, b):
    return fma_f32(a, np.float32(1), b)


# ---- the adaptive threshold -----------------------------------------------------------------------------------------------------
def _madd(x, k, acc, mutation):
    if mutation == "no_fma":
        return add_f32(mul_f32(x, k), acc)
    return fma_f32(x, k, acc)


def mean_f32(img, block=11, mutation=None):
    """The f32 Gaussian mean (before rounding) of u8 img [..., H, W]: float32 [..., H, W]."""
    _check(mutation)
    x = np.asarray(img, np.uint8).astype(np.float32)
    H, W = x.shape[-2:]
    k = gaussian_kernel_f32(block)
    r = block // 2
    if mutation == "mean_reflect101":
        ix, iy = (lambda p: reflect101(p, W)), (lambda p: reflect101(p, H))
    else:
        ix, iy = (lambda p: np.clip(p, 0, W - 1)), (lambda p: np.clip(p, 0, H - 1))
    xs, ys = np.arange(W), np.arange(H)
    col = lambda d: x[..., ix(xs + d)]
    if block <= 5 or mutation == "row_centre_first":
        acc = mul_f32(col(0), k[r])
        for j in range(1, r + 1):
            acc = _madd(add_f32(col(-j), col(j)), k[r + j], acc, mutation)
    else:
        acc = mul_f32(col(-r), k[0])
        for j in range(1, block):
            acc = _madd(col(j - r), k[j], acc, mutation)
    row = lambda d: acc[..., iy(ys + d), :]
    if mutation == "col_left_to_right":
        m = mul_f32(row(-r), k[0])
        for j in range(1, block):
            m = _madd(row(j - r), k[j], m, mutation)
    else:
        m = mul_f32(row(0), k[r])
        for j in range(1, r + 1):
            m = _madd(add_f32(row(j), row(-j)), k[r + j], m, mutation)
    return m


def round_mean(m, mutation=None):
    m = np.asarray(m, np.float32).astype(np.float64)
    v = np.floor(m + 0.5) if mutation == "round_half_away" else np.rint(m)      # m >= 0
    return np.clip(v, 0, 255).astype(np.uint8)


def adaptive_mean(img, block=11, mutation=None):
    return round_mean(mean_f32(img, block, mutation), mutation)


def idelta(c, inv, mutation=None):
    if mutation == "c_floor_ceil_swapped":
        inv = not inv
    return int(math.floor(c)) if inv else int(math.ceil(c))


def threshold_from_mean(img, mean, c=2, inv=True, mutation=None):
    d = np.asarray(img, np.int64) - np.asarray(mean, np.int64)
    t = -idelta(c, inv, mutation)
    if mutation == "lt_not_le":
        on = (d < t) if inv else (d >= t)
    else:
        on = (d <= t) if inv else (d > t)
    return np.where(on, 255, 0).astype(np.uint8)


def adaptive_threshold(img, block=11, c=2, inv=True, mutation=None):
    return threshold_from_mean(img, adaptive_mean(img, block, mutation), c, inv, mutation)


def preprocess(bgr, mutation=None):
    """preprocess_for_grid_detection of BGR u8 [..., H, W, 3] -> binary u8 [..., H, W]."""
    return adaptive_threshold(blur(gray(bgr, mutation), 5, mutation), 11, 2, True, mutation)


def preprocess_parts(bgr):
    """-> (blurred u8, f32 mean, binary) of preprocess(), for reporting a mismatching pixel."""
    b = blur(gray(bgr), 5)
    m = mean_f32(b, 11)
    return b, m, threshold_from_mean(b, round_mean(m), 2, True)


def gray_f32_formula(b, g, r):
    """The fused kernels' gray: floor(fma(b, 3735/2^15, fma(g, 19235/2^15, fma(r, 9798/2^15, 0.5)))) in f32."""
    f = lambda v: np.asarray(v, np.float32)
    t = fma_f32(f(r), np.float32(9798 / 32768), np.float32(0.5))
    t = fma_f32(f(g), np.float32(19235 / 32768), t)
    t = fma_f32(f(b), np.float32(3735 / 32768), t)
    return np.floor(t).astype(np.uint8)


# ---- tie-dense generators ------------------------------------------------------------------------------------------------------
def _weights(block):
    k = gaussian_kernel_f32(block).astype(np.float64)
    return np.outer(k, k)


def _tie_patch_linear(block, rs, offset=1.5):
    """A u8 block x block patch whose centre pixel c has a real-number mean (float taps, exact arithmetic) as close as the search
    gets to c + offset: exactly for the dyadic blocks 3/5/7, within ~1e-7 otherwise."""
    w = _weights(block)
    r = block // 2
    mask = np.ones((block, block), bool)
    mask[r, r] = False

    def start():
        p = (rs.randint(40, 200) + rs.randint(-6, 7, (block, block))).astype(np.int64)
        for _ in range(4):                               # the centre value that puts the target next to the mean
            p[r, r] = int(round(float((w * p).sum()) - offset))
        return p

    if block <= 7:
        # dyadic weights: the mean is exact in float64; greedy single steps (largest weight not above the residual) either
        # reach a residual of exactly 0 or get stuck below the smallest weight, and then a fresh start is drawn
        for _attempt in range(1000):
            p = start()
            for _ in range(400):
                e = p[r, r] + offset - float((w * p).sum())
                if e == 0:
                    return p.astype(np.uint8)
                s = int(np.sign(e))
                cand = np.where(mask & (w <= abs(e)) & (p + s >= 0) & (p + s <= 255), w, -1.0)
                if cand.max() < 0:
                    break
                p[np.unravel_index(np.argmax(cand), cand.shape)] += s
        raise AssertionError(f"no exact tie patch for block {block}")
    p = start()
    res = lambda: p[r, r] + offset - float((w * p).sum())
    # coarse greedy single steps, then one meet-in-the-middle step over pairs of (pixel, +-1) moves
    for _ in range(200):
        e = res()
        if abs(e) < w.max():
            break
        # a step may move the same pixel many times (small weights, residual up to 1/2): keep every pixel inside [1, 254], so
        # that the +-1 moves below stay inside [0, 255]
        s = int(np.sign(e))
        cand = np.where(mask & (w <= abs(e)) & (p + s >= 1) & (p + s <= 254), w, -1.0)
        if cand.max() < 0:
            break
        p[np.unravel_index(np.argmax(cand), cand.shape)] += s
    ys, xs = np.nonzero(mask)
    if len(ys) > 300:
        sel = np.sort(rs.choice(len(ys), 300, replace=False))
        ys, xs = ys[sel], xs[sel]
    n = len(ys)
    mv = np.concatenate([w[ys, xs], -w[ys, xs]])
    pix = np.concatenate([np.arange(n)] * 2)
    sgn = np.concatenate([np.ones(n, np.int64), -np.ones(n, np.int64)])
    a, b = np.triu_indices(2 * n, 1)
    keep = pix[a] != pix[b]
    a, b = a[keep], b[keep]
    order = np.argsort(mv[a] + mv[b])
    a, b = a[order], b[order]
    ps = mv[a] + mv[b]
    e = res()
    best, pick = np.inf, None
    j0 = np.searchsorted(ps, e - ps)
    for jj in (np.clip(j0 - 1, 0, len(ps) - 1), np.clip(j0, 0, len(ps) - 1)):
        err = np.abs(e - ps - ps[jj])
        distinct = ((pix[a] != pix[a[jj]]) & (pix[a] != pix[b[jj]]) & (pix[b] != pix[a[jj]]) & (pix[b] != pix[b[jj]]))
        err = np.where(distinct, err, np.inf)
        i = int(np.argmin(err))
        if err[i] < best:
            best, pick = err[i], (i, int(jj[i]))
    for q in pick:
        for m_ in (a[q], b[q]):
            p[ys[pix[m_]], xs[pix[m_]]] += sgn[m_]
    assert p.min() >= 0 and p.max() <= 255
    return p.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def tie_patches(block, count, seed):
    rs = np.random.RandomState(seed)
    return np.stack([_tie_patch_linear(block, rs) for _ in range(count)])


def tie_image(H, W, block, seed):
    """u8 [H, W]: low-contrast noise with tie patches of `block` tiled without overlap (each patch is its centre's whole window)."""
    rs = np.random.RandomState(seed)
    img = (rs.randint(60, 190) + rs.randint(-8, 9, (H, W))).astype(np.uint8)
    ny, nx = H // block, W // block
    if ny * nx == 0:
        return img
    pool = tie_patches(block, min(ny * nx, 48), seed)
    for t in range(ny * nx):
        y, x = divmod(t, nx)
        img[y * block:(y + 1) * block, x * block:(x + 1) * block] = pool[t % len(pool)]
    return img


def _blur_window_mean(g):
    """g u8 [..., 15, 15] -> (real-number mean of the centre's 11 x 11 window of the blurred patch, blurred centre)."""
    b = blur(g, 5)[..., 2:13, 2:13].astype(np.float64)
    return (b * _weights(11)).sum(axis=(-2, -1)), b[..., 5, 5]


def _tie_gray_patch(rs, tol=4e-6):
    """A 15 x 15 u8 gray patch whose blurred centre src and real-number mean satisfy |mean - (src + 1.5)| < tol.  The blur
    rounds, so the search evaluates every candidate exactly: a centre dip of the depth that comes closest, greedy single-pixel
    steps of +-1, 3, 8, then the best pairs of steps."""
    eye = np.eye(225, dtype=np.int64).reshape(225, 15, 15)
    steps = np.concatenate([s * eye for s in (1, -1, 3, -3, 8, -8)])
    dip = np.zeros((15, 15), np.int64)
    dip[6:9, 6:9] = 1

    def residual(cands):
        m, s = _blur_window_mean(np.clip(cands, 0, 255).astype(np.uint8))
        return s + 1.5 - m

    for _attempt in range(20):
        g = (rs.randint(70, 180) + rs.randint(-6, 7, (15, 15))).astype(np.int64)
        depths = np.arange(0, 16)
        rr = residual(g[None] - depths[:, None, None] * dip)
        g = g - depths[int(np.argmin(np.abs(rr)))] * dip
        e = float(residual(g[None])[0])
        for _ in range(60):
            rr = residual(g[None] + steps)
            i = int(np.argmin(np.abs(rr)))
            if abs(rr[i]) >= abs(e):
                break
            g, e = g + steps[i], float(rr[i])
            if abs(e) < 1e-3:
                break
        for _ in range(4):
            if abs(e) < tol:
                return g.astype(np.uint8)
            d = residual(g[None] + steps) - e                   # change of the residual per single step
            tot = np.abs(e + d[:, None] + d[None, :])
            ia, ib = np.unravel_index(np.argsort(tot, axis=None)[:64], tot.shape)
            cand = g[None] + steps[ia] + steps[ib]
            rr = residual(cand)
            i = int(np.argmin(np.abs(rr)))
            if abs(rr[i]) < abs(e):
                g, e = cand[i], float(rr[i])
        if abs(e) < tol:
            return g.astype(np.uint8)
    raise AssertionError("no tie patch found")


GRAY_PATCH_SEED, GRAY_PATCH_COUNT = 1, 48
CELL_SEED, CELL_COUNT = 31, 32
GRAY_PATCH_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k1_tie_patches.npz")


def make_tie_gray_patches(count=GRAY_PATCH_COUNT, seed=GRAY_PATCH_SEED):
    """The search behind tests/golden/k1_tie_patches.npz (about 0.2 s a patch): u8 [count, 15, 15]."""
    rs = np.random.RandomState(seed)
    return np.stack([_tie_gray_patch(rs) for _ in range(count)])


@functools.lru_cache(maxsize=None)
def tie_gray_patches():
    """The committed 15 x 15 gray tie patches (tests/golden/make_k1_tie_patches.py writes them with make_tie_gray_patches)."""
    return np.load(GRAY_PATCH_FILE)["gray_patches"]


def tie_frame(H, W, seed):
    """BGR u8 [H, W, 3] with B = G = R (gray = value): low-contrast noise with 15 x 15 tie patches tiled without overlap."""
    rs = np.random.RandomState(seed)
    g = (rs.randint(60, 190) + rs.randint(-8, 9, (H, W))).astype(np.uint8)
    pool = tie_gray_patches()
    ny, nx = H // 15, W // 15
    for t in range(ny * nx):
        y, x = divmod(t, nx)
        g[y * 15:(y + 1) * 15, x * 15:(x + 1) * 15] = pool[(t * 5 + seed) % len(pool)]
    return np.repeat(g[..., None], 3, axis=2)


@functools.lru_cache(maxsize=None)
def ambiguous_stripes():
    """Gray column pattern (period 7, constant down the columns) in which one column of each period has a real-number mean within
    1e-3 of src + 1.5: a 64 x 128 tile of such columns has 1/7 of its pixels ambiguous for the matrix-pipe K1 (EPS = 2^-9), more
    than its 1/8 list, so the kernel re-decides every pixel of the tile.  (Shorter periods give too few distinct means.)"""
    k = gaussian_kernel_f32(11).astype(np.float64)
    P = 7
    g = np.random.RandomState(6).randint(0, 256, (300000, P))
    ext = g[:, np.arange(-7, P + 7) % P]                             # gray columns -7 .. P+6 of the periodic pattern
    h = (16 * (ext[:, 0:P + 10] + ext[:, 4:P + 14]) + 64 * (ext[:, 1:P + 11] + ext[:, 3:P + 13]) +
         96 * ext[:, 2:P + 12])                                      # horizontal pass, columns -5 .. P+4
    b = (256 * h + 32768) >> 16                                      # the vertical pass of a column-constant image
    mean = sum(k[j] * b[:, j:j + P] for j in range(11))              # columns 0 .. P-1
    d = np.abs(mean - b[:, 5:5 + P] - 1.5).min(1)
    best = int(np.argmin(d))
    assert d[best] < 1e-3, d[best]
    return g[best].astype(np.uint8)


def stripes_frame(H, W):
    row = np.resize(ambiguous_stripes(), W)
    return np.repeat(np.broadcast_to(row, (H, W))[..., None], 3, axis=2).copy()


def grid_frame(H, W, seed):
    """A synthetic 9 x 9 grid: light noisy paper, dark lines, a few dark blobs."""
    rs = np.random.RandomState(seed)
    g = (200 + rs.randint(-12, 13, (H, W))).astype(np.int64)
    for i in range(10):
        y, x = int(0.05 * H + i * 0.1 * H), int(0.05 * W + i * 0.1 * W)
        t = 3 if i % 3 == 0 else 1
        g[max(0, y - t):y + t, int(0.05 * W):int(0.95 * W)] = 40
        g[int(0.05 * H):int(0.95 * H), max(0, x - t):x + t] = 40
    for _ in range(12):
        y, x = rs.randint(0, H), rs.randint(0, W)
        g[y:y + max(1, H // 40), x:x + max(1, W // 60)] = 30
    return np.clip(g[..., None] + rs.randint(-3, 4, (H, W, 3)), 0, 255).astype(np.uint8)


CONTENTS = ("tie", "noise", "flat", "zeros", "full", "grid", "lowcontrast", "stripes")


def content_frame(kind, H, W, seed):
    """BGR u8 [H, W, 3] of one content kind."""
    rs = np.random.RandomState(seed)
    if kind == "tie":
        return tie_frame(H, W, seed)
    if kind == "noise":
        return rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    if kind == "lowcontrast":
        return (100 + rs.randint(0, 26, (H, W, 3))).astype(np.uint8)
    if kind == "flat":
        return np.full((H, W, 3), 90 + seed % 60, np.uint8)
    if kind == "zeros":
        return np.zeros((H, W, 3), np.uint8)
    if kind == "full":
        return np.full((H, W, 3), 255, np.uint8)
    if kind == "grid":
        return grid_frame(H, W, seed)
    if kind == "stripes":
        return stripes_frame(H, W)
    raise ValueError(kind)


# ---- N1 cells ----------------------------------------------------------------------------------------------------------------------
def order_sensitive_cells(clahe, cells):
    """The cells whose CLAHE output (clahe: a function of one u8 [28, 28] cell) has a threshold(11, 2, BINARY) pixel that some
    ORDER_MUTATION flips -> (those cells, their CLAHE outputs)."""
    cl = np.stack([clahe(c) for c in cells])
    base = adaptive_threshold(cl, 11, 2, inv=False)
    hit = np.zeros(len(cells), bool)
    for m in ORDER_MUTATIONS:
        hit |= (adaptive_threshold(cl, 11, 2, inv=False, mutation=m) != base).any(axis=(1, 2))
    return cells[hit], cl[hit]


def _tie_cell(clahe, rs, tol=4e-6):
    """A 28 x 28 cell whose CLAHE output has, at its centre pixel, a real-number 11 x 11 mean within tol of src + 1.5 (CLAHE is a
    per-tile lookup table blended between tiles, so the search evaluates every candidate through `clahe`: greedy steps of +-1, 3
    on the pixels of the centre's window, then the best pairs of steps)."""
    w = _weights(11)
    eye = np.zeros((121, 28, 28), np.int64)
    eye[np.arange(121), 9 + np.arange(121) // 11, 9 + np.arange(121) % 11] = 1
    steps = np.concatenate([s * eye for s in (1, -1, 3, -3)])

    def residual(cands):
        cl = np.stack([clahe(np.clip(c, 0, 255).astype(np.uint8)) for c in cands]).astype(np.float64)
        return cl[:, 14, 14] + 1.5 - (cl[:, 9:20, 9:20] * w).sum(axis=(1, 2))

    for _attempt in range(20):
        c = (rs.randint(60, 190) + rs.randint(0, rs.randint(4, 40), (28, 28))).astype(np.int64)
        e = float(residual(c[None])[0])
        for _ in range(60):
            rr = residual(c[None] + steps)
            i = int(np.argmin(np.abs(rr)))
            if abs(rr[i]) >= abs(e):
                break
            c, e = c + steps[i], float(rr[i])
            if abs(e) < 1e-3:
                break
        for _ in range(3):
            if abs(e) < tol:
                break
            d = residual(c[None] + steps) - e
            tot = np.abs(e + d[:, None] + d[None, :])
            ia, ib = np.unravel_index(np.argsort(tot, axis=None)[:64], tot.shape)
            cand = c[None] + steps[ia] + steps[ib]
            rr = residual(cand)
            i = int(np.argmin(np.abs(rr)))
            if abs(rr[i]) < abs(e):
                c, e = cand[i], float(rr[i])
        if abs(e) < tol and c.min() >= 0 and c.max() <= 255:
            return c.astype(np.uint8)
    raise AssertionError("no tie cell found")


def make_tie_cells(clahe, count=CELL_COUNT, seed=CELL_SEED):
    """The search behind the cells of tests/golden/k1_tie_patches.npz: u8 [count, 28, 28]."""
    rs = np.random.RandomState(seed)
    return np.stack([_tie_cell(clahe, rs) for _ in range(count)])


@functools.lru_cache(maxsize=None)
def tie_cells():
    return np.load(GRAY_PATCH_FILE)["cells"]


# ---- CASES --------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    reason: str
    kind: str                       # "gray": u8 [n, H, W] for the stand-alone stages; "frame": BGR u8 [n, H, W, 3]
    make: object = None
    params: dict = field(default_factory=dict)

    def data(self):
        return self.make()


def _stripes(H, W, a, b, axis):
    v = np.where((np.arange(W if axis == 1 else H) % 2) == 0, a, b).astype(np.uint8)
    return np.broadcast_to(v[None, :] if axis == 1 else v[:, None], (H, W)).copy()


def _rand(seed, shape, lo=0, hi=256):
    return np.random.RandomState(seed).randint(lo, hi, shape).astype(np.uint8)


def _cases():
    C = []

    def add(*a, **k):
        C.append(Case(*a, **k))

    add("tie_b11", "11 x 11 tie patches: centre means within ~1e-7 of src + 1.5 (float taps): the order decides", "gray",
        lambda: np.stack([tie_image(77, 132, 11, s) for s in (1, 2)]), {"block": 11})
    add("tie_b15", "15 x 15 tie patches (block 15)", "gray", lambda: tie_image(90, 120, 15, 3)[None], {"block": 15})
    add("tie_b31", "31 x 31 tie patches (block 31)", "gray", lambda: tie_image(93, 124, 31, 4)[None], {"block": 31})
    for b in (3, 5, 7):
        add(f"tie_b{b}_half", f"block {b}: dyadic taps, exact .5 means: half to even decides", "gray",
            (lambda b=b: tie_image(8 * b, 12 * b, b, 10 + b)[None]), {"block": b})
    add("stripes_p2", "period-2 stripes of odd sum: interior means exactly x.5 for blocks 3/5/7", "gray",
        lambda: np.stack([_stripes(20, 33, 100, 103, 1), _stripes(20, 33, 7, 10, 0)]))
    add("noise_61x83", "the noise image the stand-alone stages were tested on", "gray", lambda: _rand(6, (2, 61, 83)))
    add("lowc_40x57", "low-contrast noise", "gray", lambda: _rand(8, (2, 40, 57), 100, 106))
    add("small_5x7", "5 x 7: smaller than every block > 7, borders reflected / replicated many times", "gray", lambda: _rand(9, (3, 5, 7)))
    add("one_row", "1 x 40 stripes: parity caveat pinned (full 2-D filter, see the module docstring)", "gray",
        lambda: np.stack([_stripes(1, 40, 100, 103, 1), _rand(12, (1, 40))]))
    add("one_col", "40 x 1 stripes: parity caveat pinned", "gray", lambda: np.stack([_stripes(40, 1, 100, 103, 0), _rand(13, (40, 1))]))
    add("px_1x1", "one pixel", "gray", lambda: np.array([[[0]], [[137]], [[255]]], np.uint8))
    add("px_2x2", "2 x 2: ksize 7 reflects three times", "gray", lambda: _rand(14, (3, 2, 2)))
    add("flat_gray", "flat images: the mean equals the value", "gray",
        lambda: np.stack([np.full((9, 13), v, np.uint8) for v in (0, 1, 128, 254, 255)]))
    # BGR frames for the fused kernels
    add("fused_tie", "B = G = R frames with 15 x 15 gray tie patches: blurred centre means within 4e-6 of src + 1.5", "frame",
        lambda: np.stack([tie_frame(90, 240, s) for s in (1, 2)]))
    add("fused_noise", "the noise frames test_preprocess_random_noise_bit_exact uses (RandomState(5), 3 x 75 x 140)", "frame",
        lambda: _rand(5, (3, 75, 140, 3)))
    add("fused_mixed", "tie, noise, flat, all-0, all-255, grid, low-contrast and stripes frames", "frame",
        lambda: np.stack([content_frame(k, 64, 96, i) for i, k in enumerate(CONTENTS)]))
    add("fused_2x3", "2 x 3 frames: the 5-tap blur reflects more than once", "frame", lambda: _rand(15, (2, 2, 3, 3)))
    add("fused_3x2", "3 x 2 frames", "frame", lambda: _rand(16, (2, 3, 2, 3)))
    add("fused_colour", "unequal B, G, R: the gray coefficients and rounding", "frame", lambda: _rand(17, (1, 64, 64, 3)))
    return C


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
C_VALUES = (-255, -1.5, -1, 0, 0.5, 2, 2.5, 3.999, 255)
BLOCKS = tuple(range(3, 32, 2))
