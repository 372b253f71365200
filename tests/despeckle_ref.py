"""Independent restatement of the speck filter (sv_despeckle_u8 / sv_despeckle_bits, csrc/k4_despeckle.hip) in numpy + scipy.ndimage, the
inputs that drive its flood fill to where it turns or gives up, and the table of test images built from them.  Imports nothing from the
product.

The filter: two passes over 64x64 tiles (tile origins (0,0), then (-32,-32)); in a tile, every pixel that is not 8-connected, through
the tile's own pixels, to the tile's outermost ring is erased -- unless the kernel's flood fill has not settled within its iteration cap,
in which case the tile is left as it is for that pass.

    tile_keep(tile, sides)      what a settled fill keeps, by component labelling
    fill_iterations(tile64)     how many iterations the documented schedule needs, restated from the prose at the top of the kernel file
    despeckle(img, cap, margin) -> (want, hard, unsure)

The prediction is only relied on where it does not depend on the schedule's details: a tile that needs <= margin[0] iterations is
filtered, one that needs >= margin[1] is left alone ("hard"); anything in between is "unsure" and the exact tests use inputs that have none.
"""
import numpy as np
from scipy import ndimage

T = 64
PLAIN_FIRST = 2                    # iterations that stay in the row orientation before the fill starts alternating
_EIGHT = np.ones((3, 3), bool)


# ---- what a settled fill keeps ---------------------------------------------------------------------------------------------------------

def tile_keep(tile, sides=(True, True, True, True)):
    """Pixels of `tile` (bool, at most 64x64) that are 8-connected to the tile's outer ring.  sides = (top, bottom, left, right): which
    sides of the 64x64 tile lie inside the image; a clipped tile has no ring pixels on a side the image cut off."""
    tile = np.asarray(tile, bool)
    lab, _ = ndimage.label(tile, structure=_EIGHT)
    ring = np.zeros(tile.shape, bool)
    top, bottom, left, right = sides
    if top:
        ring[0] = True
    if bottom:
        ring[-1] = True
    if left:
        ring[:, 0] = True
    if right:
        ring[:, -1] = True
    ids = np.unique(lab[ring & tile])
    return np.isin(lab, ids[ids > 0])


# ---- the iteration schedule ------------------------------------------------------------------------------------------------------------

def _fill_along_rows(f, g):
    """f, g bool [N,64,64], g subset of f: every horizontal run of f that holds a pixel of g."""
    start = f.copy()
    start[..., 1:] &= ~f[..., :-1]
    run = np.cumsum(start.reshape(-1)).reshape(f.shape)              # id of the run a foreground pixel belongs to
    hit = np.zeros(int(run.reshape(-1)[-1]) + 1, bool)
    hit[run[g]] = True
    return f & hit[run]


def _step8(g):
    """g grown by one pixel in all 8 directions, inside the tile."""
    p = np.zeros((g.shape[0], T + 2, T + 2), bool)
    p[:, 1:-1, 1:-1] = g
    rows = p[:, :-2] | p[:, 1:-1] | p[:, 2:]
    return rows[:, :, :-2] | rows[:, :, 1:-1] | rows[:, :, 2:]


def _iterations(tiles, limit=None):
    """tiles bool [N,64,64] -> (count int [N], reached bool [N,64,64]).  count = iterations run up to and including the first one that
    changed nothing; with a limit, `limit` for a tile that is still changing in iteration limit - 1 (its `reached` is then partial)."""
    f = np.ascontiguousarray(tiles, bool)
    ft = np.ascontiguousarray(f.swapaxes(1, 2))
    ring = np.zeros((T, T), bool)
    ring[0] = ring[-1] = True
    ring[:, 0] = ring[:, -1] = True
    g = _fill_along_rows(f, f & ring)                                  # the initial run fill from the ring seeds
    n = len(f)
    count = np.zeros(n, np.int64)
    live = np.ones(n, bool)
    it = 0
    while live.any() and (limit is None or it < limit):
        columns = it >= PLAIN_FIRST and (it - PLAIN_FIRST) % 2 == 0      # rows, rows, then columns, rows, columns, ...
        idx = np.flatnonzero(live)
        gi = g[idx]
        if columns:
            cur = ft[idx]
            gt = np.ascontiguousarray(gi.swapaxes(1, 2))
            g2 = _fill_along_rows(cur, gt | (cur & _step8(gt))).swapaxes(1, 2)
        else:
            cur = f[idx]
            g2 = _fill_along_rows(cur, gi | (cur & _step8(gi)))
        changed = (g2 != gi).any(axis=(1, 2))
        g[idx] = g2
        it += 1
        count[idx] = it
        live[idx[~changed]] = False
    return count, g


def fill_iterations(tile64, limit=None):
    """Iterations the documented fill schedule needs on one 64x64 tile (a clipped tile padded with zeros): the initial run fill comes from
    the ring seeds; an iteration takes one 8-neighbour step and fills along the runs of its orientation; the first PLAIN_FIRST iterations
    work along rows, after that the orientation alternates; the count includes the first iteration that changes nothing.  Where the
    schedule settles, what it reached must be what the labelling keeps."""
    tile64 = np.asarray(tile64, bool)
    assert tile64.shape == (T, T)
    count, reached = _iterations(tile64[None], limit)
    if limit is None or count[0] < limit:
        assert np.array_equal(reached[0], tile_keep(tile64)), "the fill's fixed point is not the ring-connected set"
    return int(count[0])


# ---- the whole filter ------------------------------------------------------------------------------------------------------------------

def tile_origins(H, W, off):
    return [(y0, x0) for y0 in range(-off, H, T) for x0 in range(-off, W, T)]


def _klass(count, margin):
    return 0 if count <= margin[0] else (2 if count >= margin[1] else 1)          # settles for sure, unsure, gives up for sure


def despeckle(img, cap=96, margin=(64, 150), counts=None, stages=None):
    """img bool/uint8 [H,W] -> (want bool [H,W], hard, unsure); hard and unsure are lists of (pass, y0, x0) with the tile's origin.
    A tile that needs <= margin[0] iterations is filtered, one that needs >= margin[1] is left untouched in that pass and listed in
    `hard`; a tile in between is listed in `unsure`, and `want` treats it by `cap` (filtered if it needs <= cap iterations).  What an
    unsure first-pass tile leaves behind is one of two images; a second-pass tile that sees the difference is looked at with both and is
    unsure unless both settle for sure or both give up for sure.  cap=None: the filter with no iteration cap at all.  counts: a dict that
    receives {(pass, y0, x0): iterations, clipped at margin[1]}; stages: a list that receives the image after each pass."""
    want = np.asarray(img) > 0
    alt = want.copy()                                    # first-pass result with the unsure tiles decided the other way round
    H, W = want.shape
    hard, unsure, counts_out = [], [], counts
    for p, off in enumerate((0, T // 2)):
        origins = tile_origins(H, W, off)
        boxes = [(max(y0, 0), min(y0 + T, H), max(x0, 0), min(x0 + T, W)) for y0, x0 in origins]
        sides = [(ya == y0, yb == y0 + T, xa == x0, xb == x0 + T) for (y0, x0), (ya, yb, xa, xb) in zip(origins, boxes)]
        keeps = [tile_keep(want[ya:yb, xa:xb], sd) for (ya, yb, xa, xb), sd in zip(boxes, sides)]
        if cap is None:
            for (ya, yb, xa, xb), keep in zip(boxes, keeps):
                want[ya:yb, xa:xb] = keep
            if stages is not None:
                stages.append(want.copy())
            continue

        def counts(image, which):
            padded = np.zeros((len(which), T, T), bool)
            for j, k in enumerate(which):
                (y0, x0), (ya, yb, xa, xb) = origins[k], boxes[k]
                padded[j, ya - y0:yb - y0, xa - x0:xb - x0] = image[ya:yb, xa:xb]
            c, reached = _iterations(padded, margin[1])
            for j, k in enumerate(which):
                if c[j] < margin[1]:
                    (y0, x0), (ya, yb, xa, xb) = origins[k], boxes[k]
                    assert np.array_equal(reached[j, ya - y0:yb - y0, xa - x0:xb - x0], tile_keep(image[ya:yb, xa:xb], sides[k])) \
                        and not (reached[j] & ~padded[j]).any(), "the fill's fixed point is not the ring-connected set"
            return c

        every = list(range(len(origins)))
        count = counts(want, every)
        forked = [k for k in every if not np.array_equal(want[boxes[k][0]:boxes[k][1], boxes[k][2]:boxes[k][3]],
                                                         alt[boxes[k][0]:boxes[k][1], boxes[k][2]:boxes[k][3]])] if p == 1 else []
        other = dict(zip(forked, counts(alt, forked))) if forked else {}
        if counts_out is not None:
            counts_out.update({(p, y0, x0): int(c) for (y0, x0), c in zip(origins, count)})
        new_want = want.copy()
        for k, (y0, x0) in enumerate(origins):
            ya, yb, xa, xb = boxes[k]
            kl = _klass(count[k], margin)
            doubtful = kl == 1 or (k in other and _klass(other[k], margin) != kl)
            if doubtful:
                unsure.append((p, y0, x0))
            elif kl == 2:
                hard.append((p, y0, x0))
            erase = count[k] <= cap
            if erase:
                new_want[ya:yb, xa:xb] = keeps[k]
            if p == 0:                                         # alt: as want, except that a doubtful tile goes the other way
                alt[ya:yb, xa:xb] = want[ya:yb, xa:xb] if erase == doubtful else keeps[k]
        want = new_want
        if stages is not None:
            stages.append(want.copy())
    return want, hard, unsure


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------

ORIENTATIONS = ("id", "lr", "ud", "t")


def orient(tile, how):
    """A tile as built ("id"), mirrored left-right ("lr"), mirrored upside down ("ud") or transposed ("t")."""
    return {"id": tile, "lr": tile[:, ::-1], "ud": tile[::-1], "t": tile.T}[how].copy()


def boustrophedon(ndiag, npix=None, first=None, rows=(8, 61), cols=(8, 61), how="id"):
    """One 1-pixel path in a 64x64 tile: `ndiag` diagonals x - y = c (c = first, first + 3, ...) inside the box rows x cols, joined at
    alternate ends, with a straight tail from the start of the first diagonal to the tile's left edge; npix keeps only the first npix
    pixels of the path, counted from the tail.  A 1-pixel diagonal advances one pixel per fill iteration in either orientation, so the
    fill walks the path pixel by pixel.  Outside the box only the tail is set (room for a line through the tile, or for a clipped tile)."""
    (rlo, rhi), (clo, chi) = rows, cols
    if first is None:
        first = (clo + chi) // 2 - (rlo + rhi) // 2 - 3 * (ndiag // 2) + 1
    path = []
    for k in range(ndiag):
        c = first + 3 * k
        d = [(y, y + c) for y in range(rlo, rhi + 1) if clo <= y + c <= chi]
        assert len(d) > 3, (ndiag, first, k)
        if k % 2:
            d.reverse()
        if not path:
            path += [(d[0][0], x) for x in range(0, d[0][1])]                         # the tail, from the ring inwards
        else:
            (y, x), (ty, tx) = path[-1], d[0]                                       # the link: along the row, then along the column
            step = 1 if tx > x else -1
            path += [(y, xx) for xx in range(x + step, tx + step, step)]
            step = 1 if ty > y else -1
            path += [(yy, tx) for yy in range(y + step, ty, step)]
            if path[-1] == d[0]:
                path.pop()
        path += d
    tile = np.zeros((T, T), bool)
    for y, x in path[:npix]:
        tile[y, x] = True
    return orient(tile, how)


def spiral(gap=1, how="id"):
    """A square 1-pixel spiral from the tile's top-left corner inwards, arms `gap` + 1 pixels apart."""
    tile = np.zeros((T, T), bool)
    top, bottom, left, right = 0, T - 1, 0, T - 1
    pitch = gap + 1
    while bottom - top >= 0 and right - left >= 0:
        tile[top, left:right + 1] = True
        tile[top:bottom + 1, right] = True
        if bottom - top < pitch or right - left < pitch:
            break
        tile[bottom, left + pitch:right + 1] = True
        tile[top + pitch:bottom + 1, left + pitch] = True
        top, bottom, left, right = top + pitch, bottom - pitch, left + pitch, right - pitch
    return orient(tile, how)


def noise(density, seed, shape=(T, T)):
    """Percolation noise: every pixel set with probability `density`."""
    return np.random.RandomState(seed).uniform(size=shape) < density


def place(img, y, x, tile):
    """ORs `tile` into img with its top-left pixel at (y, x); the tile has to fit."""
    h, w = tile.shape
    assert 0 <= y and 0 <= x and y + h <= img.shape[0] and x + w <= img.shape[1], (y, x, tile.shape, img.shape)
    img[y:y + h, x:x + w] |= tile
    return img


# ---- the input table -------------------------------------------------------------------------------------------------------------------
# A case is (imgs bool [n,H,W], tiles): tiles lists (frame, regime, pass, y0, x0) for every tile placed on purpose -- regime "capped"
# (>= 150 iterations in that pass), "long" (50...64) or "easy" (<= 64).  tests/test_despeckle_ref.py asserts the regimes on the CPU.

LONG_NOISE_SEEDS = (4, 27, 37, 43, 93, 100, 109, 124)            # 64x64 tiles of density-0.38 noise that need 53...61 iterations on their own


def special(kind, how="id", rows=(8, 61), cols=(8, 61), seed=0):
    """A 64x64 tile of a regime: "capped" / "long" = a path plus a lone 3x3 speck across the tile's horizontal centre line (strictly inside
    this tile, on the ring of the other pass's tiles), "spiral" (long), "noise" (long, seed from LONG_NOISE_SEEDS), "easy" = specks only."""
    if kind in ("capped", "long"):
        if kind == "capped":
            tile = boustrophedon(8, rows=rows, cols=cols)
        else:                                                      # the path length that puts the fill between 55 and 60 iterations
            for npix in range(40, 300):
                tile = boustrophedon(2, npix, rows=rows, cols=cols)
                if fill_iterations(tile) >= 55:
                    break
        if rows == (8, 61) and cols == (8, 61):
            tile[30:33, 10:13] = True
        return orient(tile, how)
    if kind == "spiral":
        return spiral(1, how)
    if kind == "noise":
        return noise(0.38, seed)
    assert kind == "easy"
    tile = np.zeros((T, T), bool)
    tile[30:33, 10:13] = True
    tile[5:8, 40:44] = True
    tile[50:52, 20:22] = True
    tile[0:4, 30] = True                                           # and something that hangs on the ring
    return orient(tile, how)


def specks(H, W, seed, per_tile=1.5):
    """A field of lone 3x3 specks, about per_tile of them per 64x64 pixels."""
    rs = np.random.RandomState(seed)
    img = np.zeros((H, W), bool)
    for _ in range(int(per_tile * H * W / (T * T)) + 1):
        y, x = rs.randint(0, max(H - 2, 1)), rs.randint(0, max(W - 2, 1))
        img[y:y + 3, x:x + 3] = True
    return img


def rectangle_outline(H, W, top, bottom, left, right, thick=3):
    img = np.zeros((H, W), bool)
    img[top:top + thick, left:right + thick] = True
    img[bottom:bottom + thick, left:right + thick] = True
    img[top:bottom + thick, left:left + thick] = True
    img[top:bottom + thick, right:right + thick] = True
    return img


def compose(H, W, items, speck_seed, outline=None, frame=0):
    """items: (regime, kind, pass, y0, x0, kwargs) -- the tile special(kind, **kwargs) with its origin at (y0, x0) on the grid of `pass`
    (clipped to the image).  Around them a field of easy specks, kept 2 px away from the placed tiles and from the outline."""
    img = np.zeros((H, W), bool)
    taken = np.zeros((H, W), bool)
    tiles = []
    for regime, kind, p, y0, x0, kw in items:
        off = p * (T // 2)
        assert (y0 + off) % T == 0 and (x0 + off) % T == 0, (y0, x0, p)
        tile = special(kind, **kw)
        ya, yb, xa, xb = max(y0, 0), min(y0 + T, H), max(x0, 0), min(x0 + T, W)
        assert not taken[ya:yb, xa:xb].any(), ("placed tiles overlap", kind, p, y0, x0)
        taken[ya:yb, xa:xb] = True
        img[ya:yb, xa:xb] |= tile[ya - y0:yb - y0, xa - x0:xb - x0]
        tiles.append((frame, regime, p, y0, x0))
    keep_off = taken.copy()
    if outline is not None:
        img |= outline
        keep_off |= outline
    keep_off = ndimage.binary_dilation(keep_off, structure=_EIGHT, iterations=2)
    img |= specks(H, W, speck_seed) & ~keep_off
    return img, tiles


def case_topology():
    """512x768, one frame: capped paths in all four orientations in tiles of the first grid and of the second, long paths, spirals and noise
    tiles beside them, easy specks everywhere else, and a rectangle outline that runs through capped and long tiles of both grids (through
    the rows or columns the paths leave free)."""
    H, W = 512, 768
    outline = rectangle_outline(H, W, 67, 474, 67, 579)
    o = lambda how: dict(how=how)
    items = [
        # first grid; the outline's top edge crosses tile row 1, its left edge tile column 1
        ("capped", "capped", 0, 64, 128, o("id")), ("long", "long", 0, 64, 256, o("lr")), ("capped", "capped", 0, 64, 384, o("lr")),
        ("capped", "capped", 0, 192, 64, o("t")), ("capped", "capped", 0, 192, 192, o("ud")), ("long", "long", 0, 192, 320, o("id")),
        ("long", "long", 0, 192, 448, o("ud")), ("long", "long", 0, 320, 64, o("t")),
        ("long", "noise", 0, 0, 640, dict(seed=4)), ("long", "noise", 0, 128, 640, dict(seed=27)),
        ("long", "spiral", 0, 448, 640, o("id")), ("long", "spiral", 0, 448, 704, o("t")),
        # second grid; the outline's bottom edge crosses the tile row at y0 = 416
        ("capped", "capped", 1, 288, 160, o("id")), ("capped", "capped", 1, 288, 288, o("t")), ("capped", "capped", 1, 288, 480, o("lr")),
        ("long", "long", 1, 352, 416, o("lr")), ("capped", "capped", 1, 416, 160, o("ud")), ("long", "long", 1, 416, 288, o("ud")),
        ("long", "spiral", 1, 288, 608, o("ud")), ("long", "spiral", 1, 352, 672, o("lr")),
        ("easy", "easy", 0, 0, 0, o("id")), ("easy", "easy", 0, 128, 128, o("lr")), ("easy", "easy", 0, 384, 512, o("t")),
    ]
    img, tiles = compose(H, W, items, 101, outline)
    return img[None], tiles


def _strip_items(layout, regimes):
    """Placed tiles of a (70, 8192) frame.  The first grid has one full tile row (128 tiles), the second grid's lower tile row starts at
    y0 = 32 (rows 32...69 exist), its first and last tiles are clipped to 32 columns; TPW = 4 tiles share a wave.  Layout 0: first-grid tiles
    0, 63 | 64 (a group boundary), second-grid tiles 3 | 4 and the clipped last one.  Layout 1: first-grid tiles 3 | 4 and 127, second-grid
    tiles 0 (clipped) and 63 | 64.  regimes: two regimes used alternately."""
    low = (2, 35)
    if layout == 0:
        first = [(0, "lr"), (63, "id"), (64, "t")]
        second = [(3, dict(how="id", rows=low)), (4, dict(how="lr", rows=low)), (128, dict(how="id", rows=low, cols=(2, 29)))]
    else:
        first = [(3, "ud"), (4, "t"), (127, "lr")]
        second = [(0, dict(how="lr", rows=low, cols=(2, 29))), (63, dict(how="lr", rows=low)), (64, dict(how="id", rows=low))]
    items = []
    for k, (j, how) in enumerate(first):
        r = regimes[k % 2]
        items.append((r, r, 0, 0, j * T, dict(how=how)))
    for k, (j, kw) in enumerate(second):
        r = regimes[(k + 1) % 2]
        items.append((r, r, 1, 32, j * T - 32, kw if r != "easy" else dict(how=kw["how"])))
    return items


def case_strip(n=2, special_frames=None):
    """(70, 8192): wider than a band of the LDS kernel holds, so sv_despeckle_bits runs the tile-per-wave kernel.  Frames listed in
    special_frames (default: all, layouts 0 and 1 in turn) carry capped and long tiles at the positions of _strip_items; with
    special_frames given, the other frames carry easy tiles at the positions of layout 0."""
    H, W = 70, 8192
    imgs, tiles = [], []
    for f in range(n):
        if special_frames is None:
            items = _strip_items(f % 2, ("capped", "long") if f % 4 < 2 else ("long", "capped"))
        else:
            items = _strip_items(0, ("capped", "long") if f in special_frames else ("easy", "easy"))
        img, t = compose(H, W, items, 300 + f, frame=f)
        imgs.append(img)
        tiles += t
    return np.stack(imgs), tiles


def case_bytes_odd():
    """(130, 250) and (67, 61), three different frames each: W % 4 != 0, so every tile of the byte kernel takes the per-pixel path, and
    H % 64 != 0 with n > 1."""
    out = []
    for H, W, seed in ((130, 250, 11), (67, 61, 12)):
        imgs, tiles = [], []
        for f in range(3):
            items = []
            if W >= 192:
                items = [[("capped", "capped", 1, 32, 32, dict(how="t")), ("long", "spiral", 0, 64, 128, dict(how="lr"))],
                         [("capped", "capped", 0, 64, 0, dict(how="lr")), ("long", "long", 1, 32, 160, dict(how="ud"))],
                         [("long", "long", 0, 0, 128, dict(how="id")), ("capped", "capped", 0, 64, 64, dict(how="ud"))]][f]
            img, t = compose(H, W, items, seed * 10 + f, frame=f)
            if not items:                                        # the small shape: noise instead, one clipped tile per side and pass
                img |= noise(0.3, seed * 100 + f, (H, W))
            imgs.append(img)
            tiles += t
        out.append((np.stack(imgs), tiles))
    return out


def case_words(H, W):
    """(200, 96) and (1080, 1920), three different frames: an odd number of words per row and W % 64 == 32 for the band kernel (200, 96);
    the production shape.  Placed tiles differ from frame to frame; the 1080p frames also carry a rectangle outline through some."""
    imgs, tiles = [], []
    for f in range(3):
        if (H, W) == (200, 96):
            items = [[("capped", "capped", 0, 0, 0, dict(how="id")), ("long", "long", 1, 96, 32, dict(how="lr"))],
                     [("capped", "capped", 0, 128, 0, dict(how="lr")), ("long", "long", 1, 32, 32, dict(how="t"))],
                     [("long", "long", 0, 0, 0, dict(how="ud")), ("capped", "capped", 1, 96, 32, dict(how="t"))]][f]
            outline = None
        else:
            outline = rectangle_outline(H, W, 64 * 2 + 3, 64 * 14 + 32 + 58, 64 * 3 + 3, 64 * 25 + 3)
            items = [("capped", "capped", 0, 128, 64 * (5 + 4 * f), dict(how="id")), ("long", "long", 0, 128, 64 * (7 + 4 * f), dict(how="lr")),
                     ("capped", "capped", 0, 64 * (5 + f), 192, dict(how="t")), ("capped", "capped", 1, 928, 64 * (6 + 3 * f) - 32, dict(how="ud")),
                     ("long", "long", 1, 928, 64 * (8 + 3 * f) - 32, dict(how="ud")),
                     ("long", "noise", 0, 64 * 8, 64 * (10 + f), dict(seed=LONG_NOISE_SEEDS[f])),
                     ("long", "spiral", 1, 64 * 9 - 32, 64 * (15 + f) - 32, dict(how=ORIENTATIONS[f])), ("capped", "capped", 1, 416, 64 * 12 - 32, dict(how=ORIENTATIONS[f + 1]))]
        img, t = compose(H, W, items, 500 + f, outline, frame=f)
        imgs.append(img)
        tiles += t
    return np.stack(imgs), tiles


def case_independence(H, W):
    """Five frames; only frame 2 holds capped and long tiles, frames 1 and 3 hold easy tiles at the same positions, frames 0 and 4 specks."""
    if (H, W) == (70, 8192):
        return case_strip(5, special_frames=(2,))
    assert (H, W) == (192, 288)
    where = [(0, 64, 64), (0, 0, 192), (1, 96, 160), (1, 96, 224), (0, 128, 0)]
    imgs, tiles = [], []
    for f in range(5):
        if f == 2:
            items = [(r, r, p, y, x, dict(how=h)) for (p, y, x), r, h in zip(where, ("capped", "long", "capped", "long", "capped"), ("id", "t", "ud", "lr", "t"))]
        elif f in (1, 3):
            items = [("easy", "easy", p, y, x, dict(how="id")) for p, y, x in where]
        else:
            items = []
        img, t = compose(H, W, items, 700 + f, frame=f)
        imgs.append(img)
        tiles += t
    return np.stack(imgs), tiles


NEAR_CAP_SEEDS = (5, 6, 7)


def case_near_cap():
    """Three 1080p frames of percolation noise at density 0.38, just below the 8-connected percolation threshold: the natural input closest
    to the cap (tiles that need 65...95 iterations turn up; none over 96 in 6,000 tiles of the model)."""
    return np.stack([noise(0.38, s, (1080, 1920)) for s in NEAR_CAP_SEEDS])
