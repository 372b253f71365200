"""numpy restatement of the arithmetic of cv/preprocess_v2.py as DESIGN.md section 2 states it, independent of the kernels
(csrc/k7_preprocess_v2.hip) and of the drop-in's host code: the GPU tests compare both against it bit for bit, and
tests/test_preprocess_v2_ref.py holds it against scipy.ndimage and the C oracle from the other side.

Everything is integer, or float32 / float64 with one rounding per operation (numpy never fuses)."""
import math

import numpy as np

GAUSS21_SIGMA = 0.3 * ((21 - 1) * 0.5 - 1) + 0.8          # 3.5


# ---- borders ----------------------------------------------------------------------------------------------------------------
def reflect101_index(p, n):
    """cv2.borderInterpolate(p, n, BORDER_REFLECT_101) for an integer array p: reflect repeatedly until inside."""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    period = 2 * n - 2
    m = np.mod(p, period)
    return np.where(m < n, m, period - m)


def pad_reflect101(img, top, bottom, left, right):
    H, W = img.shape
    ys = reflect101_index(np.arange(-top, H + bottom), H)
    xs = reflect101_index(np.arange(-left, W + right), W)
    return img[ys[:, None], xs[None, :]]


# ---- 1-2: structuring elements and morphology ------------------------------------------------------------------------------
def ellipse_half_widths(k):
    """dx per row of cv2.getStructuringElement(MORPH_ELLIPSE, (k, k))."""
    r = c = k // 2
    inv_r2 = 1.0 / (r * r) if r else 0.0
    out = []
    for i in range(k):
        dy = i - r
        out.append(int(np.rint(c * math.sqrt((r * r - dy * dy) * inv_r2))))     # np.rint: half to even
    return out


def structuring_element(shape, k):
    """shape 'rect' or 'ellipse' -> u8 [k,k] of 0/1."""
    el = np.zeros((k, k), np.uint8)
    if shape == "rect":
        el[:] = 1
        return el
    c = k // 2
    for i, dx in enumerate(ellipse_half_widths(k)):
        el[i, max(c - dx, 0):min(c + dx + 1, k)] = 1
    return el


def _sliding_extreme(a, length, fn):
    """out[:, x] = fn over a[:, x : x + length] for x = 0 .. a.shape[1] - length (van Herk / Gil-Werman: two running
    extremes over blocks of `length`)."""
    if length == 1:
        return a
    H, Wp = a.shape
    nb = -(-Wp // length)
    ident = 0 if fn is np.maximum else 255
    b = np.full((H, nb * length), ident, a.dtype)
    b[:, :Wp] = a
    blocks = b.reshape(H, nb, length)
    fwd = fn.accumulate(blocks, axis=2).reshape(H, -1)
    bwd = fn.accumulate(blocks[:, :, ::-1], axis=2)[:, :, ::-1].reshape(H, -1)
    n = Wp - length + 1
    return fn(bwd[:, :n], fwd[:, length - 1:length - 1 + n])


def _morph(img, el, fn):
    """dst(x,y) = fn over src(x + j - ax, y + i - ay) for el[i,j] = 1, anchor (k//2, k//2), element unreflected; pixels
    outside the image do not take part."""
    k = el.shape[0]
    ax = ay = k // 2
    H, W = img.shape
    ident = 0 if fn is np.maximum else 255
    pad = np.full((H + 2 * k, W + 2 * k), ident, np.uint8)
    pad[k:k + H, k:k + W] = img
    out = np.full((H, W), ident, np.uint8)
    spans = {}
    for i in range(k):
        ones = np.flatnonzero(el[i])
        if ones.size:
            assert ones[-1] - ones[0] + 1 == ones.size          # one run per row
            spans.setdefault((int(ones[0]), int(ones.size)), []).append(i)
    for (j0, length), rows in spans.items():
        # slid[:, x'] covers padded columns x' .. x' + length - 1; pixel x needs x + k + j0 - ax
        slid = _sliding_extreme(pad, length, fn)
        cols = slice(k + j0 - ax, k + j0 - ax + W)
        for i in rows:
            r0 = k + i - ay
            out = fn(out, slid[r0:r0 + H, cols])
    return out


def dilate(img, el):
    return _morph(img, el, np.maximum)


def erode(img, el):
    return _morph(img, el, np.minimum)


def morph_close(img, el):
    return erode(dilate(img, el), el)


def morph_open(img, el):
    return dilate(erode(img, el), el)


# ---- 3-4: box mean, glare, shadow ---------------------------------------------------------------------------------------------
def window_sums(img, k, square=False):
    """Exact integer k x k window sums (BORDER_REFLECT_101), k odd."""
    r = k // 2
    p = pad_reflect101(img, r, r, r, r).astype(np.int64)
    if square:
        p = p * p
    c = np.zeros((p.shape[0] + 1, p.shape[1] + 1), np.int64)
    c[1:, 1:] = p.cumsum(0).cumsum(1)
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


def box_mean(img, k):
    """cv2.blur(img, (k, k)) on u8: round to nearest of the exact mean (k*k odd: no ties)."""
    S = window_sums(img, k)
    return ((2 * S + k * k) // (2 * k * k)).astype(np.uint8)


def illumination_kernel_size(shape):
    k = max(shape) // 10
    k += k % 2 == 0
    return max(k, 51)


def shadow_kernel_size(shape):
    k = max(shape) // 20
    k += k % 2 == 0
    return k


def detect_glare(gray, threshold=250):
    mask = gray > threshold
    ratio = float(np.count_nonzero(mask)) / float(mask.size)
    return bool(ratio > 0.01), mask.astype(np.uint8) * 255


def detect_shadow(gray):
    mean = box_mean(gray, shadow_kernel_size(gray.shape))
    mask = (gray.astype(np.int32) - mean.astype(np.int32)) < -30
    ratio = float(np.count_nonzero(mask)) / float(mask.size)
    return bool(0.05 < ratio < 0.5), mask.astype(np.uint8) * 255


# ---- 5: GaussianBlur(21, 21, 0) -------------------------------------------------------------------------------------------------
def gauss21_taps():
    """The 21 taps in 8 fractional bits: error diffusion from the ends inward, centre = 256 - the rest."""
    s = GAUSS21_SIGMA
    t = [math.exp(-((i - 10) ** 2) / (2 * s * s)) for i in range(21)]
    tot = math.fsum(t)
    t = [v / tot for v in t]
    out, err = [0] * 21, 0.0
    for i in range(10):
        a = t[i] * 256 + err
        v = int(np.rint(a))
        err = a - v
        out[i] = out[20 - i] = v
    out[10] = 256 - 2 * sum(out[:10])
    return out


def gaussian_blur21(img):
    taps = gauss21_taps()
    H, W = img.shape
    p = pad_reflect101(img, 10, 10, 10, 10).astype(np.int64)
    h = sum(taps[j] * p[:, j:j + W] for j in range(21))
    v = sum(taps[j] * h[j:j + H, :] for j in range(21))
    return ((v + (1 << 15)) >> 16).astype(np.uint8)


# ---- 6: division ----------------------------------------------------------------------------------------------------------------
def divide_normalize(gray, background):
    b = np.maximum(background, 1).astype(np.float32)
    q = gray.astype(np.float32) / b
    return (q * np.float32(255)).clip(0, 255).astype(np.uint8)


def normalize_illumination(gray):
    el = structuring_element("ellipse", illumination_kernel_size(gray.shape))
    return divide_normalize(gray, morph_close(gray, el))


def remove_shadow(gray):
    return divide_normalize(gray, gaussian_blur21(dilate(gray, structuring_element("ellipse", 7))))


# ---- 7: CLAHE -------------------------------------------------------------------------------------------------------------------
def clahe_extend(img, tiles_x, tiles_y):
    """The image CLAHE really works on: extended at the bottom / right to a multiple of the tile grid (REFLECT_101)."""
    H, W = img.shape
    eb = tiles_y - H % tiles_y if H % tiles_y else 0
    er = tiles_x - W % tiles_x if W % tiles_x else 0
    return pad_reflect101(img, 0, eb, 0, er) if (eb or er) else img


def _clahe_divisible(src, clip, tiles_x, tiles_y):
    H, W = src.shape
    tw, th = W // tiles_x, H // tiles_y
    area = tw * th
    lut_scale = np.float32(255.0) / np.float32(area)
    clip_limit = max(int(clip * area / 256), 1) if clip > 0 else 0
    luts = np.empty((tiles_y, tiles_x, 256), np.float32)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            hist = np.bincount(src[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256).astype(np.int64)
            if clip_limit > 0:
                clipped = int(np.maximum(hist - clip_limit, 0).sum())
                hist = np.minimum(hist, clip_limit)
                batch, residual = divmod(clipped, 256)
                hist = hist + batch
                if residual:
                    step = max(256 // residual, 1)
                    idx = np.arange(0, 256, step)[:residual]
                    hist[idx] += 1
            cdf = hist.cumsum().astype(np.float32)
            luts[ty, tx] = np.clip(np.rint(cdf * lut_scale), 0, 255)
    one, half = np.float32(1), np.float32(0.5)

    def axis(n, tile, tiles):
        t = np.arange(n, dtype=np.float32) * (one / np.float32(tile)) - half
        t1 = np.floor(t).astype(np.int32)
        a = t - t1.astype(np.float32)
        return np.maximum(t1, 0), np.minimum(t1 + 1, tiles - 1), a, one - a

    ty1, ty2, ya, ya1 = axis(H, th, tiles_y)
    tx1, tx2, xa, xa1 = axis(W, tw, tiles_x)
    v = src.astype(np.intp)
    Y1, Y2, X1, X2 = ty1[:, None], ty2[:, None], tx1[None, :], tx2[None, :]
    top = luts[Y1, X1, v] * xa1[None, :] + luts[Y1, X2, v] * xa[None, :]
    bot = luts[Y2, X1, v] * xa1[None, :] + luts[Y2, X2, v] * xa[None, :]
    res = top * ya1[:, None] + bot * ya[:, None]
    assert res.dtype == np.float32
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


def clahe(img, clip=2.0, tiles=(8, 8)):
    """cv2.createCLAHE(clip, tiles).apply(img), tiles = (tiles_x, tiles_y)."""
    H, W = img.shape
    return _clahe_divisible(clahe_extend(img, tiles[0], tiles[1]), clip, tiles[0], tiles[1])[:H, :W]


# ---- 8: Otsu --------------------------------------------------------------------------------------------------------------------
def otsu_threshold(gray):
    h = np.bincount(gray.ravel(), minlength=256)
    scale = 1.0 / float(gray.size)
    mu = 0.0
    for i in range(256):
        mu += i * float(h[i])
    mu *= scale
    mu1 = q1 = max_sigma = 0.0
    max_val = 0
    eps = float(np.finfo(np.float32).eps)
    for i in range(256):
        p_i = float(h[i]) * scale
        mu1 *= q1
        q1 += p_i
        q2 = 1.0 - q1
        if min(q1, q2) < eps or max(q1, q2) > 1.0 - eps:
            continue
        mu1 = (mu1 + i * p_i) / q1
        mu2 = (mu - q1 * mu1) / q2
        sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
        if sigma > max_sigma:
            max_sigma, max_val = sigma, i
    return max_val


def threshold_otsu(gray):
    return np.where(gray > otsu_threshold(gray), 0, 255).astype(np.uint8)


# ---- 9: Sauvola -----------------------------------------------------------------------------------------------------------------
def sauvola_threshold_from_sums(s1, s2, window, k):
    """The float32 threshold of a pixel from its exact window sums of g and g^2 (int64 arrays of any one shape)."""
    inv = 1.0 / float(window * window)
    mean = (np.asarray(s1).astype(np.float64) * inv).astype(np.float32)
    sq = (np.asarray(s2).astype(np.float64) * inv).astype(np.float32)
    var = np.maximum(sq - mean * mean, np.float32(0))
    std = np.sqrt(var)
    t = mean * (np.float32(1) + np.float32(k) * (std / np.float32(128) - np.float32(1)))
    assert t.dtype == np.float32
    return t


def threshold_sauvola(gray, window=25, k=0.2):
    t = sauvola_threshold_from_sums(window_sums(gray, window), window_sums(gray, window, square=True), window, k)
    return np.where(gray.astype(np.float32) < t, 255, 0).astype(np.uint8)


# ---- the existing K1 stages the module reuses: the C oracle restates them -----------------------------------------------------
def _oracle():
    import sv_oracle
    return sv_oracle


def threshold_adaptive(gray, block=11, c=2, inv=True):
    return _oracle().adaptive_threshold(gray, block, c, inv)


def blur5(gray):
    return _oracle().gaussian_blur(gray, 5)


def grayscale(image):
    return image if image.ndim == 2 else _oracle().gray(image)


# ---- 10-11: the module's pipelines ------------------------------------------------------------------------------------------------
def morphological_cleanup(binary, close_size=3, open_size=2):
    if close_size > 0:
        binary = morph_close(binary, structuring_element("rect", close_size))
    if open_size > 0:
        binary = morph_open(binary, structuring_element("rect", open_size))
    return binary


def score_binary(b):
    ratio = (255.0 * float(np.count_nonzero(b)) / float(b.size)) / 255.0
    if ratio < 0.02 or ratio > 0.3:
        return 0
    return 1 - abs(ratio - 0.1) / 0.1


def preprocess_for_grid_detection(image, use_illumination_norm=True, use_shadow_removal=True):
    gray = grayscale(image)
    has_shadow, _ = detect_shadow(gray)
    enhanced = gray
    if has_shadow and use_shadow_removal:
        enhanced = remove_shadow(enhanced)
    if use_illumination_norm:
        enhanced = normalize_illumination(enhanced)
    enhanced = clahe(enhanced, 2.0, (8, 8))
    return morphological_cleanup(threshold_adaptive(blur5(enhanced), 11, 2), 3, 2)


def preprocess_multi_strategy(image):
    """-> dict with the fields of PreprocessResult."""
    gray = grayscale(image)
    has_glare, _ = detect_glare(gray)
    has_shadow, _ = detect_shadow(gray)
    illum = normalize_illumination(gray)
    normalized = normalize_illumination(remove_shadow(gray)) if has_shadow else illum
    enhanced = clahe(normalized, 2.0, (8, 8))
    blurred = blur5(enhanced)
    cands = [("adaptive", morphological_cleanup(threshold_adaptive(blurred, 11, 2))),
             ("otsu", morphological_cleanup(threshold_otsu(blurred))),
             ("sauvola", morphological_cleanup(threshold_sauvola(blurred, 25, 0.2)))]
    best, best_score = 0, score_binary(cands[0][1])
    for i in (1, 2):
        s = score_binary(cands[i][1])
        if s > best_score:
            best, best_score = i, s
    return dict(binary=cands[best][1], gray=gray, enhanced=enhanced, illumination_normalized=illum, has_glare=has_glare,
                has_shadow=has_shadow, method_used=cands[best][0])


def preprocess_cell(cell, clip_limit=2.0, tile_size=4):
    gray = grayscale(cell)
    return threshold_adaptive(clahe(gray, clip_limit, (tile_size, tile_size)), 11, 2, inv=False)
