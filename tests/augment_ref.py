"""The contract of K22 (sv_augment_u8, include/sudoku_vision_hip.h): a numpy restatement of every step kind from its step record,
of Philox4x32-10 and of the random fields.  Written from the header's text, with plain array expressions and no helper shared with
the product; where tests/grid_v2_ref.py and tests/warp_ref.py already state a piece of cv2's arithmetic (the affine coordinates, the
weight table, resize) that statement is used.

cv2 is not available, so parity with OpenCV itself is unpinned (as for grid_v2_ref.py)."""
import numpy as np

import grid_v2_ref
import warp_ref

F = np.float32
MAX_STEPS, MAX_SIDE, MAX_RADIUS = 10, 64, 16
NONE, AFFINE, PERSPECTIVE, BRIGHTNESS, CONTRAST, BLUR, SCALE, FILL_RECT, ELASTIC, NOISE_GAUSS, NOISE_SP = range(11)
# 96 bytes: int32 op, int32 i[5], then 72 bytes that are double d[9] or float f[18]
STEP_DTYPE = np.dtype({"names": ["op", "i", "d", "f"], "formats": ["<i4", ("<i4", (5,)), ("<f8", (9,)), ("<f4", (18,))], "offsets": [0, 4, 24, 24], "itemsize": 96})


def step(op, i=(), d=(), f=()):
    """One step record."""
    s = np.zeros((), STEP_DTYPE)
    s["op"] = op
    s["i"][:len(i)] = i
    if len(f):
        s["f"][:len(f)] = f
    else:
        s["d"][:len(d)] = d
    return s


def program(chains):
    """chains: a list of lists of step records -> (steps [n, MAX_STEPS], n_steps int32 [n])."""
    steps = np.zeros((len(chains), MAX_STEPS), STEP_DTYPE)
    for k, c in enumerate(chains):
        for j, s in enumerate(c):
            steps[k, j] = s
    return steps, np.array([len(c) for c in chains], np.int32)


# ---- Philox4x32-10 and the fields -----------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Salmon et al., SC'11.  Counter words as uint64 arrays holding 32-bit values (broadcast); -> four uint32 arrays."""
    m = np.uint64(0xffffffff)
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & m for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xffffffff, int(k1) & 0xffffffff
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c1, c3, c0, c2 = p1 & m, p0 & m, n0, n2
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def field_words(seed, index, slot, salt, H, W):
    """The random block of every pixel of output `index`'s step slot: uint32 [H, W, 4]."""
    seed, index = int(seed) & (2 ** 64 - 1), int(index)
    pixel = np.arange(H * W, dtype=np.uint64)
    w = philox4x32_10(pixel, index & 0xffffffff, ((index >> 32) << 8) | (slot & 255), int(salt) & 0xffffffff, seed & 0xffffffff, seed >> 32)
    return np.stack(w, -1).reshape(H, W, 4)


def uniform_pm1(word):
    return (word >> np.uint32(8)).astype(F) * F(2.0 ** -23) - F(1)


def uniform01(word):
    return word.astype(np.float64) * 2.0 ** -32


def normal(w0, w1):
    u1 = (w0.astype(np.float64) + 1.0) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * uniform01(w1))


# ---- host helpers ---------------------------------------------------------------------------------------------------------
def rotation_matrix(center, angle, scale=1.0):
    return grid_v2_ref.rotation_matrix(center, angle, scale)


def perspective_matrix(src, dst):
    """cv2.getPerspectiveTransform on float32 points: the 8x8 elimination with partial pivoting in OpenCV's order, Python floats
    (one rounding per operation).  None for a degenerate system."""
    src, dst = np.asarray(src, F).reshape(4, 2), np.asarray(dst, F).reshape(4, 2)
    a = [[0.0] * 9 for _ in range(8)]
    for i in range(4):
        sx, sy, dx, dy = float(src[i, 0]), float(src[i, 1]), float(dst[i, 0]), float(dst[i, 1])
        a[i] = [sx, sy, 1.0, 0.0, 0.0, 0.0, -sx * dx, -sy * dx, dx]
        a[i + 4] = [0.0, 0.0, 0.0, sx, sy, 1.0, -sx * dy, -sy * dy, dy]
    for i in range(8):
        piv = i
        for j in range(i + 1, 8):
            if abs(a[j][i]) > abs(a[piv][i]):
                piv = j
        if not abs(a[piv][i]) >= 2.220446049250313e-16 * 100:
            return None
        a[i], a[piv] = a[piv], a[i]
        d = -1 / a[i][i]
        for j in range(i + 1, 8):
            alpha = a[j][i] * d
            for k in range(i + 1, 9):
                a[j][k] += alpha * a[i][k]
    for i in range(7, -1, -1):
        s = a[i][8]
        for k in range(i + 1, 8):
            s -= a[i][k] * a[k][8]
        a[i][8] = s / a[i][i]
    return np.array([a[i][8] for i in range(8)] + [1.0]).reshape(3, 3)


def elastic_radius(sigma):
    return (int(np.rint(sigma * 8 + 1)) | 1) // 2


def elastic_taps(sigma):
    """-> (radius r, float32 taps [r + 1] by distance) of cv2.GaussianBlur((0, 0), sigma) on a float32 image."""
    r = elastic_radius(sigma)
    scale2x = -0.125 / (sigma * sigma)
    v = [float(np.exp(np.float64(4 * j * j) * scale2x)) for j in range(r + 1)]
    total = 0.0
    for j in range(r, 0, -1):
        total += v[j]
    total *= 2.0
    total += 1.0
    inv = 1.0 / total
    return r, np.array([inv] + [v[j] * inv for j in range(1, r + 1)], np.float64).astype(F)


# ---- the steps --------------------------------------------------------------------------------------------------------------
def sample_replicate(img, X, Y):
    """cv2's bilinear tap sum at the 1/32-pixel positions X, Y (int64 arrays), BORDER_REPLICATE: every tap clamped into the image."""
    if grid_v2_ref._TAB is None:
        grid_v2_ref._TAB = grid_v2_ref._bilinear_table()
    H, W = img.shape
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    w = grid_v2_ref._TAB[Y & 31, X & 31]
    acc = np.zeros(X.shape, np.int64)
    for t, (oy, ox) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        acc += img[np.clip(sy + oy, 0, H - 1), np.clip(sx + ox, 0, W - 1)].astype(np.int64) * w[..., t]
    return ((acc + 16384) >> 15).astype(np.uint8)


def warp_affine(img, M):
    """cv2.warpAffine(img, M, (w, h), INTER_LINEAR, BORDER_REPLICATE), M the forward 2x3."""
    H, W = img.shape
    X, Y = grid_v2_ref.warp_coords(np.asarray(M, np.float64).reshape(2, 3), (W, H))
    return sample_replicate(img, X, Y)


def invert3(S):
    """cv::invert of a 3x3 in double: cofactors times 1 / det, a singular matrix -> zeros."""
    S = [float(v) for v in np.asarray(S, np.float64).reshape(9)]
    c0, c1, c2 = S[4] * S[8] - S[5] * S[7], S[3] * S[8] - S[5] * S[6], S[3] * S[7] - S[4] * S[6]
    det = (S[0] * c0 - S[1] * c1) + S[2] * c2
    det = 1.0 / det if det != 0 else 0.0
    return [c0 * det, (S[2] * S[7] - S[1] * S[8]) * det, (S[1] * S[5] - S[2] * S[4]) * det,
            (S[5] * S[6] - S[3] * S[8]) * det, (S[0] * S[8] - S[2] * S[6]) * det, (S[2] * S[3] - S[0] * S[5]) * det,
            c2 * det, (S[1] * S[6] - S[0] * S[7]) * det, (S[0] * S[4] - S[1] * S[3]) * det]


def perspective_coords(Minv, H, W):
    """warp_ref.coords for an H x W destination of at most 64 columns (one block, origin column 0): -> X, Y in 1/32 px."""
    M = [float(v) for v in Minv]
    y = np.arange(H, dtype=np.float64)[:, None]
    x1 = np.arange(W, dtype=np.float64)[None, :]
    X0 = (M[0] * 0.0 + M[1] * y) + M[2]
    Y0 = (M[3] * 0.0 + M[4] * y) + M[5]
    W0 = (M[6] * 0.0 + M[7] * y) + M[8]
    Wd = W0 + M[6] * x1
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Wr = np.where(Wd != 0, 32.0 / np.where(Wd != 0, Wd, 1.0), 0.0)
        fX = np.clip((X0 + M[0] * x1) * Wr, warp_ref.INT_MIN, warp_ref.INT_MAX)
        fY = np.clip((Y0 + M[3] * x1) * Wr, warp_ref.INT_MIN, warp_ref.INT_MAX)
    return np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)


def warp_perspective(img, M):
    """cv2.warpPerspective(img, M, (w, h), INTER_LINEAR, BORDER_REPLICATE), M the forward 3x3."""
    H, W = img.shape
    X, Y = perspective_coords(invert3(M), H, W)
    return sample_replicate(img, X, Y)


def brightness(img, delta):
    return np.clip(img.astype(F) + F(delta), 0, 255).astype(np.uint8)


def contrast(img, factor):
    mean = float(int(img.astype(np.int64).sum())) / float(img.size)
    return np.clip((img.astype(np.float64) - mean) * float(factor) + mean, 0, 255).astype(np.uint8)


def blur(img, k):
    if k == 1:
        return img.copy()
    taps = {3: [1, 2, 1], 5: [1, 4, 6, 4, 1]}[k]
    r = k // 2
    H, W = img.shape
    p = np.pad(img.astype(np.int64), r, mode="reflect")
    h = sum(t * p[:, j:j + W] for j, t in enumerate(taps))
    s = sum(t * h[j:j + H] for j, t in enumerate(taps))
    return ((s + 8) >> 4 if k == 3 else (s + 128) >> 8).astype(np.uint8)


def scale(img, new_w, new_h, crop):
    H, W = img.shape
    scaled = warp_ref.resize(img, (new_w, new_h))
    if crop:
        y0, x0 = (new_h - H) // 2, (new_w - W) // 2
        return scaled[y0:y0 + H, x0:x0 + W].copy()
    out = np.full((H, W), 128, np.uint8)
    y0, x0 = (H - new_h) // 2, (W - new_w) // 2
    out[y0:y0 + new_h, x0:x0 + new_w] = scaled
    return out


def fill_rect(img, x, y, ew, eh, value):
    out = img.copy()
    out[y:y + eh, x:x + ew] = value
    return out


def field_blur(field, taps):
    """Rows, then columns; REFLECT_101; acc = t[-r]*v[-r], then + t[j]*v[j] for j = -r+1 .. r, each product and sum one float32 rounding."""
    r = len(taps) - 1
    H, W = field.shape
    out = field.astype(F)
    for axis in (1, 0):
        pad = [(0, 0), (0, 0)]
        pad[axis] = (r, r)
        p = np.pad(out, pad, mode="reflect")
        n = out.shape[axis]
        acc = None
        for j in range(-r, r + 1):
            sl = [slice(None), slice(None)]
            sl[axis] = slice(r + j, r + j + n)
            term = F(taps[abs(j)]) * p[tuple(sl)]
            acc = term if acc is None else acc + term
        out = acc.astype(F)
    return out


def remap(img, map_x, map_y):
    """cv2.remap(INTER_LINEAR, BORDER_REPLICATE) with float32 maps."""
    X = np.clip(np.rint((map_x.astype(F) * F(32)).astype(np.float64)), warp_ref.INT_MIN, warp_ref.INT_MAX).astype(np.int64)
    Y = np.clip(np.rint((map_y.astype(F) * F(32)).astype(np.float64)), warp_ref.INT_MIN, warp_ref.INT_MAX).astype(np.int64)
    return sample_replicate(img, X, Y)


def elastic_fields(words, alpha, taps):
    """-> the displacements dx, dy (float32 [H, W]) from a block of random words."""
    return field_blur(uniform_pm1(words[..., 0]), taps) * F(alpha), field_blur(uniform_pm1(words[..., 1]), taps) * F(alpha)


def elastic(img, words, alpha, taps):
    H, W = img.shape
    dx, dy = elastic_fields(words, alpha, taps)
    x, y = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    return remap(img, x + dx, y + dy)


def noise_gauss_values(img, words, sigma):
    """The float64 values before the clip and the truncation."""
    return img.astype(np.float64) + float(sigma) * normal(words[..., 0], words[..., 1])


def noise_gauss(img, words, sigma):
    return np.clip(noise_gauss_values(img, words, sigma), 0, 255).astype(np.uint8)


def noise_sp(img, words, half):
    out = img.copy()
    out[uniform01(words[..., 0]) < float(half)] = 255
    out[uniform01(words[..., 1]) < float(half)] = 0
    return out


def apply_step(img, s, seed=0, index=0, slot=0):
    """One step record on one u8 image."""
    op, i, d, f = int(s["op"]), [int(v) for v in s["i"]], s["d"], s["f"]
    H, W = img.shape
    if op == AFFINE:
        return warp_affine(img, d[:6])
    if op == PERSPECTIVE:
        return warp_perspective(img, d)
    if op == BRIGHTNESS:
        return brightness(img, d[0])
    if op == CONTRAST:
        return contrast(img, d[0])
    if op == BLUR:
        return blur(img, i[0])
    if op == SCALE:
        return scale(img, i[0], i[1], i[2])
    if op == FILL_RECT:
        return fill_rect(img, *i)
    if op in (ELASTIC, NOISE_GAUSS, NOISE_SP):
        words = field_words(seed, index, slot, i[4], H, W)
        if op == ELASTIC:
            return elastic(img, words, f[0], f[1:2 + i[0]])
        return noise_gauss(img, words, d[0]) if op == NOISE_GAUSS else noise_sp(img, words, d[0])
    return img.copy()


def run_program(src, steps, n_steps, src_index, seed=0, index_base=0):
    """sv_augment_u8: src u8 [n_src, H, W] -> u8 [n_out, H, W]."""
    src = np.asarray(src, np.uint8)
    out = np.empty((len(n_steps),) + src.shape[1:], np.uint8)
    for o in range(len(n_steps)):
        img = src[min(max(int(src_index[o]), 0), len(src) - 1)]
        for slot in range(min(max(int(n_steps[o]), 0), MAX_STEPS)):
            img = apply_step(img, steps[o, slot], seed, index_base + o, slot)
        out[o] = img
    return out


# ---- inputs: never constant, so that a replicated and a constant border differ ------------------------------------------------
def sample_image(H, W, seed=0):
    """A diagonal gradient plus noise, bright corners included."""
    rs = np.random.RandomState(1000 + seed)
    y, x = np.mgrid[0:H, 0:W]
    g = (x * 255.0 / max(W - 1, 1) * 0.6 + y * 255.0 / max(H - 1, 1) * 0.4)
    return np.clip(g + rs.randint(-40, 41, (H, W)), 0, 255).astype(np.uint8)


def sample_images(n, H, W, seed=0):
    return np.stack([sample_image(H, W, seed * 100 + k) for k in range(n)])
