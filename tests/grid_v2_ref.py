"""The contract of the cv/grid_v2.py drop-in: a numpy / pure-Python restatement of the arithmetic that
include/sudoku_vision_hip.h states for sv_harris_corners_u8, sv_warp_affine_u8, sv_hough_lines_p_u8 and
sv_find_grid_corners_v2_u8, and of detect_grid's control flow (reference cv/grid_v2.py:401-508).

Written separately from the kernels and the host library: plain loops and array expressions, no helper shared with the
product.  The contour primitives (findContours, contourArea, arcLength, approxPolyDP) come from the C oracle
(oracle/sv_oracle.py), which the v1 corner search is already pinned against.

cv2 is not available, so parity with OpenCV itself is unpinned (as for preprocess_v2_ref.py)."""
import math

import numpy as np

F = np.float32


# ---- Harris corners: cv2.goodFeaturesToTrack(useHarrisDetector=True, blockSize=3) --------------------------------------
def harris_response(gray, k=0.04):
    """gray u8 [H,W] -> float32 [H,W].  Every array expression below is one float32 rounding per element."""
    g = np.asarray(gray, np.uint8).astype(F)
    p = np.pad(g, 1, mode="reflect")                         # BORDER_REFLECT_101
    scale = 1.0 / (4 * 3 * 255)
    k0, k1 = F(scale), F(2 * scale)
    sx = p[:, 2:] - p[:, :-2]                                # row pass of Dx on the H+2 padded rows
    dx = k1 * sx[1:-1] + k0 * (sx[:-2] + sx[2:])
    sy = k1 * p[:, 1:-1] + k0 * (p[:, :-2] + p[:, 2:])       # row pass of Dy
    dy = sy[2:] - sy[:-2]

    def box(a):                                              # unnormalised 3x3 sum in double, rounded to float32 once
        q = np.pad(a, 1, mode="reflect").astype(np.float64)
        h = (q[:, :-2] + q[:, 1:-1]) + q[:, 2:]
        return ((h[:-2] + h[1:-1]) + h[2:]).astype(F)

    a, b, c = box(dx * dx), box(dx * dy), box(dy * dy)
    t = a + c
    return (a * c - b * b) - (F(k) * t) * t


def harris_candidates(resp, quality_level):
    """-> list of (response, y, x) in selection order: the thresholded image's 3x3 maxima, strongest first, ties raster."""
    H, W = resp.shape
    mx = resp.max()
    if not mx > 0:
        return []
    t = float(quality_level) * float(mx)
    thr = np.where(resp.astype(np.float64) < t, F(0), resp)
    d = np.full((H + 2, W + 2), -np.inf, F)                  # dilate: only in-image neighbours take part
    d[1:-1, 1:-1] = thr
    dil = thr.copy()
    for j in range(3):
        for i in range(3):
            dil = np.maximum(dil, d[j:j + H, i:i + W])
    keep = (thr != 0) & (thr == dil)
    keep[0, :] = keep[-1, :] = False
    keep[:, 0] = keep[:, -1] = False
    ys, xs = np.nonzero(keep)
    cand = [(float(thr[y, x]), int(y), int(x)) for y, x in zip(ys, xs)]
    cand.sort(key=lambda c: (-c[0], c[1], c[2]))
    return cand


def harris_corners(gray, max_corners=100, quality_level=0.01, min_distance=10, k=0.04, window=None):
    """-> (corners float32 [m,2] as (x, y), response float32 [H,W], number of candidates).
    window: MUTANT -- a candidate is compared with the first `window` kept corners only."""
    resp = harris_response(gray, k)
    cand = harris_candidates(resp, quality_level)
    kept = np.zeros((max(min(len(cand), int(max_corners)), 1), 2), np.int64)          # (x, y) of the corners kept so far
    n = 0
    md2 = int(min_distance) * int(min_distance)
    for _, y, x in cand:
        if n >= max_corners:
            break
        d = kept[:n if window is None else min(n, window)] - (x, y)
        if ((d * d).sum(axis=1) >= md2).all():
            kept[n] = (x, y)
            n += 1
    return kept[:n].astype(F), resp, len(cand)


# ---- cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT) on u8 ------------------------------------------------------------------
def _bilinear_table():
    """cv2's int16 table of 32x32 x 4 weights, built the way cv2 builds it: float32 products, saturate to int16, and where the
    four do not sum to 32768 the difference goes to the largest (sum too small) or smallest (too large) of the entries cv2
    examines -- for the 2x2 kernel those are flat indices 3..6 from the entry's base, which reach into the zero-initialised
    entries behind it."""
    tab = np.zeros(32 * 32 * 4 + 8, np.int64)
    one = [(F(1) - F(i) * F(1 / 32), F(i) * F(1 / 32)) for i in range(32)]
    for i in range(32):
        for j in range(32):
            base = (i * 32 + j) * 4
            isum = 0
            for k1 in range(2):
                for k2 in range(2):
                    v = F(one[i][k1] * one[j][k2]) * F(32768)
                    w = int(min(max(np.rint(v), -32768), 32767))
                    tab[base + k1 * 2 + k2] = w
                    isum += w
            if isum != 32768:
                diff = isum - 32768
                big = small = 3
                for k1 in (1, 2):
                    for k2 in (1, 2):
                        q = k1 * 2 + k2
                        if tab[base + q] < tab[base + small]:
                            small = q
                        elif tab[base + q] > tab[base + big]:
                            big = q
                tab[base + (big if diff < 0 else small)] -= diff
    return tab[:4096].reshape(32, 32, 4)


_TAB = None


def _sat_int(v):
    return np.clip(np.rint(v), -2147483648.0, 2147483647.0).astype(np.int64)


def _sat_int_half_away(v):
    """MUTANT of _sat_int: a tie goes away from zero (C's lround), not to the even neighbour."""
    v = np.asarray(v, np.float64)
    return np.clip(np.sign(v) * np.floor(np.abs(v) + 0.5), -2147483648.0, 2147483647.0).astype(np.int64)


def _sat_int_truncating(v):
    """MUTANT of _sat_int: the fraction is dropped (a C cast)."""
    return np.clip(np.trunc(v), -2147483648.0, 2147483647.0).astype(np.int64)


WARP_ROUNDINGS = {"half_even": _sat_int, "half_away": _sat_int_half_away, "truncate": _sat_int_truncating}


def _wrap32(v):
    return ((v + 2 ** 31) % 2 ** 32) - 2 ** 31


def invert_affine(M):
    """cv2.warpAffine's inversion of the forward matrix, this sequence of double operations."""
    m = [float(v) for v in np.asarray(M, np.float64).reshape(6)]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m1, m3 = m[1] * -D, m[3] * -D
    b1 = -A11 * m[2] - m1 * m[5]
    b2 = -m3 * m[2] - A22 * m[5]
    return [A11, m1, b1, m3, A22, b2]


def warp_coords(M, dsize, rounding="half_even"):
    """-> (X, Y) int64 [h,w]: the source position of every destination pixel in 1/32 px (cell X >> 5, fraction X & 31).
    rounding: WARP_ROUNDINGS; anything but "half_even" is a mutant."""
    sat = WARP_ROUNDINGS[rounding]
    dw, dh = dsize
    m = invert_affine(M)
    xs = np.arange(dw, dtype=np.float64)
    ys = np.arange(dh, dtype=np.float64)
    adelta = sat(m[0] * xs * 1024.0)
    bdelta = sat(m[3] * xs * 1024.0)
    X0 = _wrap32(sat((m[1] * ys + m[2]) * 1024.0) + 16)
    Y0 = _wrap32(sat((m[4] * ys + m[5]) * 1024.0) + 16)
    X = _wrap32(X0[:, None] + adelta[None, :]) >> 5
    Y = _wrap32(Y0[:, None] + bdelta[None, :]) >> 5
    return X, Y


def warp_affine(src, M, dsize, border_value=0, rounding="half_even"):
    """src u8 [H,W], M forward 2x3, dsize (w, h) -> u8 [h,w]."""
    global _TAB
    if _TAB is None:
        _TAB = _bilinear_table()
    src = np.asarray(src, np.uint8)
    H, W = src.shape
    dw, dh = dsize
    X, Y = warp_coords(M, dsize, rounding)
    sx = np.clip(X >> 5, -32768, 32767)
    sy = np.clip(Y >> 5, -32768, 32767)
    w = _TAB[Y & 31, X & 31]                                 # [dh,dw,4]
    acc = np.zeros((dh, dw), np.int64)
    for t, (oy, ox) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        ty, tx = sy + oy, sx + ox
        inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        px = np.where(inside, src[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)].astype(np.int64), int(border_value))
        acc += px * w[:, :, t]
    return ((acc + 16384) >> 15).astype(np.uint8)


def rotation_matrix(center, angle, scale=1.0):
    """cv2.getRotationMatrix2D."""
    a = angle * (math.pi / 180)                              # cv2: angle *= CV_PI / 180
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    return np.array([[alpha, beta, (1 - alpha) * center[0] - beta * center[1]],
                     [-beta, alpha, beta * center[0] + (1 - alpha) * center[1]]], np.float64)


def enlarged_box(shape, angle):
    """Rotation about the integer centre into the bounding box of the turned frame: -> (forward matrix, (width, height))."""
    height, width = shape
    fwd = rotation_matrix((width // 2, height // 2), angle)
    c, s = np.abs(fwd[0, :2])
    box = (int(height * s + width * c), int(height * c + width * s))
    fwd[:, 2] += [(box[0] - width) / 2, (box[1] - height) / 2]
    return fwd, box


def rotate_image(image, angle, border_value=255):
    """-> (the frame turned by `angle` degrees into its enlarged box, the forward matrix)."""
    fwd, box = enlarged_box(image.shape[:2], angle)
    return warp_affine(image, fwd, box, border_value), fwd


# ---- cv2.HoughLinesP ----------------------------------------------------------------------------------------------------
def rng_outputs(count, state=2 ** 64 - 1):
    out = []
    for _ in range(count):
        state = (state & 0xffffffff) * 4164903690 + (state >> 32)
        out.append(state & 0xffffffff)
    return out


def hough_lines_p(binary, rho=1.0, theta=np.pi / 180, threshold=100, min_line_length=50, max_line_gap=10):
    """-> list of (x0, y0, x1, y1) in the order the lines are found."""
    img = np.asarray(binary)
    H, W = img.shape
    rho, theta = F(rho), F(theta)
    irho = F(1) / rho
    numangle = int(np.rint(np.pi / float(theta)))
    numrho = int(np.rint(F((W + H) * 2 + 1) / rho))
    accum = np.zeros((numangle, numrho), np.int64)
    ang = np.arange(numangle, dtype=np.float64) * float(theta)
    tcos = (np.cos(ang) * float(irho)).astype(F)
    tsin = (np.sin(ang) * float(irho)).astype(F)
    mask = img != 0
    ys, xs = np.nonzero(mask)                                # raster order
    nz = list(zip(xs.tolist(), ys.tolist()))
    mask = mask.copy()
    half = (numrho - 1) // 2
    rows = np.arange(numangle)
    state = 2 ** 64 - 1
    lines = []

    def bins(x, y):
        return np.rint(F(x) * tcos + F(y) * tsin).astype(np.int64) + half

    def rnd(v):                                              # cvRound of a float32
        return int(np.rint(v))

    count = len(nz)
    while count > 0:
        state = (state & 0xffffffff) * 4164903690 + (state >> 32)
        idx = (state & 0xffffffff) % count
        x, y = nz[idx]
        nz[idx] = nz[count - 1]
        count -= 1
        if not mask[y, x]:
            continue
        r = bins(x, y)
        accum[rows, r] += 1
        votes = accum[rows, r]
        max_n = int(np.argmax(votes))                        # the first maximum
        if votes[max_n] < threshold:
            continue
        a, b = -tsin[max_n], tcos[max_n]
        shift = 16
        x0, y0 = x, y
        if abs(a) > abs(b):
            xflag = True
            dx0 = 1 if a > 0 else -1
            dy0 = rnd(b * F(1 << shift) / abs(a))
            y0 = (y0 << shift) + (1 << (shift - 1))
        else:
            xflag = False
            dy0 = 1 if b > 0 else -1
            dx0 = rnd(a * F(1 << shift) / abs(b))
            x0 = (x0 << shift) + (1 << (shift - 1))
        ends = [None, None]
        for k in range(2):
            gap, px, py = 0, x0, y0
            dx, dy = (dx0, dy0) if k == 0 else (-dx0, -dy0)
            while True:
                j1, i1 = (px, py >> shift) if xflag else (px >> shift, py)
                if j1 < 0 or j1 >= W or i1 < 0 or i1 >= H:
                    break
                if mask[i1, j1]:
                    gap = 0
                    ends[k] = (j1, i1)
                else:
                    gap += 1
                    if gap > max_line_gap:
                        break
                px += dx
                py += dy
        good = abs(ends[1][0] - ends[0][0]) >= min_line_length or abs(ends[1][1] - ends[0][1]) >= min_line_length
        for k in range(2):
            px, py = x0, y0
            dx, dy = (dx0, dy0) if k == 0 else (-dx0, -dy0)
            while True:
                j1, i1 = (px, py >> shift) if xflag else (px >> shift, py)
                if mask[i1, j1]:
                    if good:
                        accum[rows, bins(j1, i1)] -= 1
                    mask[i1, j1] = False
                if (j1, i1) == ends[k]:
                    break
                px += dx
                py += dy
        if good:
            lines.append((ends[0][0], ends[0][1], ends[1][0], ends[1][1]))
    return lines


# ---- the host heuristics: what cv/grid_v2.py's functions compute, stated in this file's own terms ---------------------------------
def order_points(pts):
    """The point with the least x+y, the least y-x, the greatest x+y, the greatest y-x (first one on ties), float32 [4,2]."""
    pts = np.asarray(pts)
    keys = (lambda q: q[0] + q[1], lambda q: q[1] - q[0])
    picks = []
    for key, better in ((keys[0], np.less), (keys[1], np.less), (keys[0], np.greater), (keys[1], np.greater)):
        best = 0
        for i in range(1, len(pts)):
            if better(key(pts[i]), key(pts[best])):
                best = i
        picks.append(best)
    return pts[picks].astype(F)


def _length(v):
    return np.sqrt(F(v[0] * v[0]) + F(v[1] * v[1]))


def is_valid_quadrilateral(corners, min_angle=45, max_angle=135):
    """float32 throughout, one rounding per operation: every interior angle within the limits, longest side <= 2 * shortest."""
    c = np.asarray(corners, F)
    if c.shape != (4, 2):
        return False
    edges = [c[(i + 1) % 4] - c[i] for i in range(4)]
    for i in range(4):                                       # the angle at vertex i+1, between the edge arriving and the edge leaving
        back, ahead = -edges[i], edges[(i + 1) % 4]
        inner = F(F(back[0] * ahead[0]) + F(back[1] * ahead[1]))
        cosine = inner / F(F(_length(back) * _length(ahead)) + F(1e-6))
        degrees = F(np.arccos(min(max(cosine, F(-1)), F(1)))) * F(180.0 / np.pi)
        if not (min_angle <= degrees <= max_angle):
            return False
    lengths = sorted(_length(e) for e in edges)
    return bool(lengths[-1] <= F(2) * lengths[0])


def detect_grid_contour(binary, min_area_ratio=0.1):
    import sv_oracle as o
    floor = min_area_ratio * binary.shape[0] * binary.shape[1]
    ranked = sorted(((o.contour_area(c), c) for c in o.find_contours(binary)), key=lambda t: -t[0])      # stable: ties keep cv2's order
    for area, contour in ranked:
        if area < floor:
            return None
        poly = np.asarray(o.approx_poly_dp(contour, 0.02 * o.arc_length(contour, True), True)).reshape(-1, 2)
        if len(poly) == 4 and is_valid_quadrilateral(poly.astype(F)):
            return order_points(poly.astype(F))
    return None


def _heading(line):
    return math.degrees(math.atan2(line[3] - line[1], line[2] - line[0]))


def cluster_lines_by_angle(lines, angle_tolerance=10):
    """-> (near-horizontal, near-vertical) lines; a heading is taken modulo 180 degrees."""
    groups = ([], [])
    for line in lines:
        h = _heading(line) % 180
        off_axis = (min(h, 180 - h), abs(h - 90))
        for group, off in zip(groups, off_axis):
            if off < angle_tolerance:
                group.append(tuple(line))
                break
    return groups


def line_intersection(l1, l2):
    """Cramer's rule on the two lines through the segments' ends; None when the determinant vanishes."""
    (ax, ay, bx, by), (cx, cy, dx, dy) = [[int(v) for v in l] for l in (l1, l2)]
    det = (ax - bx) * (cy - dy) - (ay - by) * (cx - dx)
    if abs(det) < 1e-6:
        return None
    t = ((ax - cx) * (cy - dy) - (ay - cy) * (cx - dx)) / det
    return (ax + t * (bx - ax), ay + t * (by - ay))


def find_grid_from_lines(horizontal, vertical, image_shape):
    if min(len(horizontal), len(vertical)) < 2:
        return None
    mid_y = [(l[1] + l[3]) / 2 for l in horizontal]
    mid_x = [(l[0] + l[2]) / 2 for l in vertical]
    top, bottom = horizontal[int(np.argmin(mid_y))], horizontal[len(mid_y) - 1 - int(np.argmax(mid_y[::-1]))]   # first least, last greatest
    left, right = vertical[int(np.argmin(mid_x))], vertical[len(mid_x) - 1 - int(np.argmax(mid_x[::-1]))]
    crossings = [line_intersection(a, b) for a, b in ((top, left), (top, right), (bottom, right), (bottom, left))]
    if None in crossings:
        return None
    quad = np.array(crossings, F)
    limit = np.array([image_shape[1], image_shape[0]]) + 50
    return quad if ((quad >= -50) & (quad <= limit)).all() else None


def detect_grid_lines(binary):
    unit = min(binary.shape) // 10
    lines = hough_lines_p(binary, threshold=50, min_line_length=unit, max_line_gap=unit // 5)
    quad = find_grid_from_lines(*cluster_lines_by_angle(lines), binary.shape) if len(lines) >= 4 else None
    return order_points(quad) if quad is not None and is_valid_quadrilateral(quad) else None


def detect_rotation_angle(binary):
    lines = hough_lines_p(binary, threshold=30, min_line_length=30, max_line_gap=5)
    if len(lines) < 2:
        return 0.0
    folded = np.array([_heading(l) % 90 for l in lines])
    return float(np.median(np.where(folded > 45, folded - 90, folded)))


def polygon_area_f32(pts):
    """Shoelace area of float32 points, accumulated in double from the closing edge on."""
    p = [(float(x), float(y)) for x, y in np.asarray(pts, F)]
    twice = 0.0
    for (x0, y0), (x1, y1) in zip(p[-1:] + p[:-1], p):
        twice += x0 * y1 - y0 * x1
    return abs(twice * 0.5)


def fit_quadrilateral_ransac(corners, image_shape, n_iterations=100, inlier_threshold=10):
    """The best-scoring of n_iterations random 4-subsets (one np.random.choice each, drawn first): a valid quadrilateral covering
    at least a tenth of the image scores (area share + shortest/longest side) / 2, float32 side lengths, the score in double."""
    if len(corners) < 4:
        return None
    frame_area = image_shape[0] * image_shape[1]
    winner = (0, None)
    for draw in [np.random.choice(len(corners), 4, replace=False) for _ in range(n_iterations)]:
        quad = order_points(corners[draw])
        share = polygon_area_f32(quad) / frame_area
        if not is_valid_quadrilateral(quad) or share < 0.1:
            continue
        lengths = sorted(float(_length(quad[(i + 1) % 4] - quad[i])) for i in range(4))
        value = share * 0.5 + lengths[0] / (lengths[-1] + 1e-6) * 0.5
        if value > winner[0]:
            winner = (value, quad)
    return winner[1]


def detect_grid(binary, gray=None, try_rotation=True, try_multiple_methods=True):
    """The four methods as a table, tried in order -> dict(corners, confidence, method, rotation_angle, debug_info)."""
    debug = {}

    def by_rotation():
        if not try_rotation:
            return None
        debug["detected_rotation"] = angle = detect_rotation_angle(binary)
        if abs(angle) <= 2:
            return None
        turned, fwd = rotate_image(binary, angle)
        quad = detect_grid_contour(turned)
        if quad is None:
            return None
        back = np.array(invert_affine(fwd)).reshape(2, 3)    # the inverse affine map takes the corners home
        return (back @ np.column_stack([quad, [1.0] * 4]).T).T.astype(F), angle

    def by_corners():
        if gray is None:
            return None
        found = harris_corners(gray)[0]
        debug["harris_corners"] = len(found)
        return fit_quadrilateral_ransac(found, binary.shape) if len(found) >= 4 else None

    table = [("contour", 0.9, lambda: detect_grid_contour(binary)), ("lines", 0.8, lambda: detect_grid_lines(binary)),
             ("contour_rotated", 0.7, by_rotation), ("harris_ransac", 0.6, by_corners)]
    for method, confidence, run in table if try_multiple_methods else table[:1]:
        quad, angle = run(), 0
        if isinstance(quad, tuple):
            quad, angle = quad
        if quad is not None:
            return {"corners": quad, "confidence": confidence, "method": method, "rotation_angle": angle, "debug_info": debug}
    return {"corners": None, "confidence": 0, "method": "none", "rotation_angle": 0, "debug_info": debug}


# ---- inputs of the hard-case tests: tests/test_grid_v2_ref.py states on the CPU what each one does to the restatement, --------------
# ---- tests/test_gpu_grid_v2.py runs them through K13 ------------------------------------------------------------------------------
def noise(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


# k_harris_response's tile is 64 x 16 (pixel halo 2, derivative halo 1): exact tiles, then last tiles one, two, one and three pixels
# high and one, two, one and 63 wide, whose reflected halo lies inside the neighbouring tile's area
TILING_SHAPES = ((16, 64), (17, 65), (18, 66), (33, 129), (19, 127))


def corner_squares(shape, inset=1, level=30, value=255):
    """A bright 2x2 square `inset` pixels from both borders in each image corner: every response that is not zero lies in the last tile's
    reflected halo.  inset 1 gives one candidate per corner; inset 0 puts the maximum on pixel (0, 0) and leaves no candidate."""
    img = np.full(shape, level, np.uint8)
    lo, hi = slice(inset, inset + 2), slice(-inset - 2, -inset or None)
    img[lo, lo] = img[lo, hi] = img[hi, lo] = img[hi, hi] = value
    return img


def border_maximum_frame():
    """20x30, level 10: [0,0] = 255 puts the frame maximum on the outermost pixel frame, which is never a candidate; a faint L of
    three pixels near the middle is the only thing the threshold can leave."""
    img = np.full((20, 30), 10, np.uint8)
    img[0, 0] = 255
    img[10, 15] = img[11, 15] = img[11, 16] = 60
    return img


def checkerboard(shape=(96, 96), period=8):
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return (((yy // period) + (xx // period)) % 2 * 255).astype(np.uint8)


def wide_range_noise(shape=(48, 80), seed=11):
    """Noise whose left half has its contrast cut to two grey levels: at quality_level = 0 the candidates span eleven orders of magnitude."""
    img = noise(shape, seed)
    half = shape[1] // 2
    img[:, :half] = 128 + (img[:, :half] & 1)
    return img


MANY = ((192, 256), 1)             # noise(*MANY): 2771 candidates at quality_level 0.01, so the bitonic sort runs on P = 4096 keys
OVER_CAP = ((224, 320), 2)         # 4156 candidates: more than SV_HARRIS_MAX_CORNERS = 4096
POWER_OF_TWO = ((20, 67), 1)       # exactly 64 candidates: no padding key is written


def uneven_batch():
    """Three frames of MANY's shape whose candidate counts differ by more than a factor of ten each: noise (2771), a checkerboard of
    period 32 (140), two squares (8)."""
    shape = MANY[0]
    few = np.full(shape, 40, np.uint8)
    for (y, x), v in (((20, 30), 255), ((170, 200), 200)):
        few[y:y + 2, x:x + 2] = v
    return np.stack([noise(*MANY), checkerboard(shape, 32), few])


def square_column(height, squares, width=5, level=40):
    """A frame `width` wide: one 2x2 square per (row, value) at columns 1..2, rows row-1..row.  Its response has two equal maxima,
    at (x, y) = (2, row-1) and (2, row); raster order takes the upper one first."""
    img = np.full((height, width), level, np.uint8)
    for row, value in squares:
        img[row - 1:row + 1, 1:3] = value
    return img


TALL = 65600                                                    # more rows than 16 bits count
TALL_SQUARES = ((10, 200), (30000, 180), (65546, 255))          # the strongest lies exactly 65536 rows below the first
TALL_PAIR = ((65546, 255), (65550, 200), (100, 180))            # two squares 4 rows apart, both beyond row 65536
LIMIT = 65535                                                   # the tallest frame sv_harris_corners_u8 takes
LIMIT_SQUARES = ((10, 200), (30000, 180), (65520, 255), (65524, 190), (32762, 220), (32770, 210))    # rows with bit 15 set; a pair 4 and a pair 8 apart


# the affine warp
FRACTION_SOURCES = {"period 1": checkerboard((36, 36), 1), "period 3": checkerboard((36, 36), 3)}       # 0 and 255 only
FRACTION_DSIZE = (72, 72)


def fraction_sweep_matrix():
    """Forward matrix whose inverse is the scale 33/32 with the translation (-1.5, -1.40625): a step of one destination pixel moves the
    source position by 33/32 px, so the fraction walks through all 32 values, in x and in y, inside the source and beyond each border."""
    s = 32.0 / 33.0
    return np.array([[s, 0, 1.5 * s], [0, s, 1.40625 * s]], np.float64)


TIE_DSIZE = (512, 4)
_T = 33.0 / 2048                   # M3 * x * 1024 = -16.5 x: a tie at every odd x


def tie_cases():
    """name -> (source, forward matrix, the mutant rounding it shows).  Every inverse is exact in double.
    A tie shows only where the two roundings land on different sides of a multiple of 32 (X = (X0 + adelta) >> 5, X0 = ... + 16):
    * delta: Y0 = 1024 y + 16 and bdelta = rint(-16.5 x) is even at a tie, so Y0 + bdelta is even, and so is the nearest multiple of 32:
      the neighbour one below (half away from zero) can cross it, the neighbour one above (truncation) cannot -- on this matrix
      truncation and half-to-even give the same pixels, whatever the source.
    * delta, odd: the same with 1/1024 px of translation, Y0 = 1024 y + 17: now only truncation can cross.
    * translation: b1 = -16.5/1024 (half-to-even -16, away -17: X0 = 0 or -1) and b2 = 15.5/1024 (half-to-even 16, truncated 15:
      Y0 = 32 or 31), so each mutant moves every pixel by 1/32 px, one in x and one in y."""
    rows = np.zeros((12, 520), np.uint8)
    rows[::2] = 255
    return {"delta": (rows, np.array([[1, 0, 0], [_T, 1, 0]], np.float64), "half_away"),
            "delta, odd": (rows, np.array([[1, 0, 0], [_T, 1, -1.0 / 1024]], np.float64), "truncate"),
            "translation": (checkerboard((12, 520), 1), np.array([[1, 0, 16.5 / 1024], [0, 1, -15.5 / 1024]], np.float64), "both")}


DEGENERATE_MATRICES = {
    "singular": [[2, 4, 1], [1, 2, 3]],                        # D = 0: the inverse is all zeros, every pixel is src[0,0]
    "far": [[1, 0, 1e12], [0, 1, 0]],                          # sat_int saturates, the cell clamps to -32768: all border
    "tiny": [[1e-7, 0, 0], [0, 1e-7, 0]],                      # adelta and Y0 saturate at 2^31 - 1; + 16 and X0 + adelta wrap in int32
    "flip": [[-1, 0, 12.25], [0, -0.75, 6.5]],                 # negative scale
}

