"""The default glyphs of the solution overlay (Context.render_overlay, csrc/k16_overlay.hip): a stroke font of this project's own
design.  Each digit is a few polylines on a 2 x 4 grid (x right, y down); nothing comes from a font file, from OpenCV's Hershey
tables or from the reference.

default_atlas() rasterises them in numpy float64 into the 8-bit coverage atlas sv_set_overlay_glyphs takes, uint8 [9,50,50], glyph
d-1 for digit d: with dist the distance from a texel's centre to the nearest segment,
    alpha = clip(rint(255 * (HALF_WIDTH + 0.5 - dist)), 0, 255)
-- full coverage up to HALF_WIDTH - 0.5 from the stroke's axis, a one-texel linear ramp after it.  The grid maps into texels
X0..X1 by Y0..Y1, so every texel with alpha > 0 lies within 3..46 and the margin the kernel relies on is zero."""
import numpy as np

CELL = 50
HALF_WIDTH = 2.0
X0, X1, Y0, Y1 = 15.0, 35.0, 8.0, 42.0          # where grid x = 0, 2 and y = 0, 4 land, in texels

# digit -> polylines of (x, y) grid points
STROKES = {
    1: [[(0.4, 1.0), (1.2, 0.0), (1.2, 4.0)]],
    2: [[(0.0, 0.0), (2.0, 0.0), (2.0, 2.0), (0.0, 4.0), (2.0, 4.0)]],
    3: [[(0.0, 0.0), (2.0, 0.0), (2.0, 4.0), (0.0, 4.0)], [(0.6, 2.0), (2.0, 2.0)]],
    4: [[(0.0, 0.0), (0.0, 2.0), (2.0, 2.0)], [(2.0, 0.0), (2.0, 4.0)]],
    5: [[(2.0, 0.0), (0.0, 0.0), (0.0, 2.0), (2.0, 2.0), (2.0, 4.0), (0.0, 4.0)]],
    6: [[(2.0, 0.0), (0.0, 0.0), (0.0, 4.0), (2.0, 4.0), (2.0, 2.0), (0.0, 2.0)]],
    7: [[(0.0, 0.0), (2.0, 0.0), (0.7, 4.0)]],
    8: [[(0.0, 0.0), (2.0, 0.0), (2.0, 4.0), (0.0, 4.0), (0.0, 0.0)], [(0.0, 2.0), (2.0, 2.0)]],
    9: [[(2.0, 2.0), (0.0, 2.0), (0.0, 0.0), (2.0, 0.0), (2.0, 4.0), (0.0, 4.0)]],
}


def segments(digit):
    """The line segments of a digit in texel coordinates: float64 [m,2,2] as (point, (x, y))."""
    out = []
    for line in STROKES[digit]:
        pts = [(X0 + (X1 - X0) * x / 2.0, Y0 + (Y1 - Y0) * y / 4.0) for x, y in line]
        out += [(p, q) for p, q in zip(pts[:-1], pts[1:])]
    return np.array(out, np.float64)


def glyph(digit):
    """uint8 [50,50]: the coverage of one digit."""
    yy, xx = np.mgrid[0:CELL, 0:CELL].astype(np.float64)
    p = np.stack([xx, yy], -1)                                   # texel centres, (x, y)
    dist = np.full((CELL, CELL), np.inf)
    for a, b in segments(digit):
        ab = b - a
        t = np.clip(((p - a) @ ab) / (ab @ ab), 0.0, 1.0)
        near = a + t[..., None] * ab
        dist = np.minimum(dist, np.sqrt(((p - near) ** 2).sum(-1)))
    return np.clip(np.rint(255.0 * (HALF_WIDTH + 0.5 - dist)), 0, 255).astype(np.uint8)


def default_atlas():
    """uint8 [9,50,50]: glyph d-1 draws digit d."""
    return np.stack([glyph(d) for d in range(1, 10)])
