"""GPU (-m gpu): every kernel of the perspective-warp family bit-exact against tests/warp_ref.py (itself bit-exact with the C
oracle, tests/test_warp_ref.py) over warp_ref.GEOMETRIES: k_warp_perspective<1|3>, k_extract_cells, k_warp_cells, the fused
k_preprocess_warp_fused, k_grid_line_coverage<u8|bits> and k_resize_linear.  Batches mix geometries frame by frame and are
compared frame by frame; padded rows and frame gaps; and Context methods on views equal the same data made contiguous.

Only device tensors of the expected dtype reach a Context method here: the view cases stay inside their allocation even where
the row pitch is taken wrongly."""
import functools

import numpy as np
import pytest
import torch

import cnn_oracle
import warp_ref as R
from sudoku_vision_amd import _native
from sudoku_vision_amd.runtime import Context

pytestmark = pytest.mark.gpu


def _minv(g, S):
    """The product's destination -> source map of geometry g at output size S (identity for a degenerate quad)."""
    if g.minv is not None:
        return g.minv
    m, ok = Context.corners_to_minv_batch(g.corners[None], S, g.inset)
    assert bool(ok[0]) != g.degenerate, g.name
    return m[0]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want, what, minv=None, S=None):
    """Bit-exact, or an assertion naming the first mismatching pixel and (for a warp) its (sx, sy, a, b) from warp_ref."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if bad.size:
        p = tuple(bad[0])
        info = ""
        if minv is not None:
            sx, sy, a, b, _, _ = R.coords(minv, S)
            info = f" (sx, sy, a, b) = {(sx[p[0], p[1]], sy[p[0], p[1]], a[p[0], p[1]], b[p[0], p[1]])}"
        raise AssertionError(f"{what}: {len(bad)} mismatches, first at {p}: got {got[p]} want {want[p]}{info}")


@pytest.mark.parametrize("g", R.GEOMETRIES, ids=lambda g: g.name)
def test_warp_perspective(ctx, g):
    M = _minv(g, g.S)
    md = _dev(M)
    for ch in (3, 1):
        img = R.frame(g, ch)
        _same(ctx.warp_perspective(_dev(img), md, g.S), R.warp(img, M, g.S), f"{g.name} C={ch}", M, g.S)


EXTRACT = [(28, 0.1), (32, 0.2), (28, 0.0)]


@pytest.mark.parametrize("g", R.GEOMETRIES, ids=lambda g: g.name)
def test_extract_cells_on_the_warps(ctx, g):
    M = _minv(g, g.S)
    img = R.frame(g, 3)
    warped = ctx.warp_perspective(_dev(img), _dev(M), g.S)
    ref = R.warp(img, M, g.S)
    gray = R.bgr_to_gray(ref)
    for cs, ratio in EXTRACT:
        mh = int((g.S // 9) * ratio)
        _same(ctx.extract_cells(warped, cs, mh, mh), R.extract(ref, cs, ratio), f"{g.name} extract {cs},{ratio}")
    _same(ctx.extract_cells(_dev(gray), 28, int((g.S // 9) * 0.1), int((g.S // 9) * 0.1)), R.extract(gray, 28, 0.1), f"{g.name} gray")


def test_extract_cells_lds_limit(ctx):
    """A 266 x 266 crop (2400 / 9 with no margin) does not fit in 64 KiB of LDS: an error, not a launch."""
    with pytest.raises(_native.NativeError):
        ctx.extract_cells(torch.zeros((2400, 2400), dtype=torch.uint8, device="cuda"), 28, 0, 0)
    big = torch.zeros((2250, 2250), dtype=torch.uint8, device="cuda")           # 250 x 250: fits
    assert ctx.extract_cells(big, 28, 0, 0).shape == (81, 28, 28)


# ---- batches: one launch, a different geometry in every frame ------------------------------------------------------------------
BH, BW = 270, 480


# the first seven frames already mix the hardest kinds: degenerate, saturating, W = 0, strong perspective, border, ties, tiny
_FIRST = ["diamond", "huge_out", "w_zero", "persp_strong", "part_out", "tie_order", "tiny_20"]
BATCH_GEOMS = [R.BY_NAME[k] for k in _FIRST] + [g for g in R.GEOMETRIES if g.name not in _FIRST]


@functools.lru_cache(maxsize=None)
def _batch_case(i):
    """Frame i of the batch tests: geometry BATCH_GEOMS[i % len] scaled toward a BH x BW frame (maps given directly stay as they
    are), its own noise -> (frame u8 [BH,BW,3], corners float32 [4,2] or None, minv or None, binary u8 [BH,BW])."""
    g = BATCH_GEOMS[i % len(BATCH_GEOMS)]
    rs = np.random.RandomState(1000 + i)
    frame = rs.randint(0, 256, (BH, BW, 3), dtype=np.uint8)
    binary = np.where(rs.randint(0, 7, (BH, BW)) == 0, 255, 0).astype(np.uint8)
    if g.minv is not None:
        return frame, None, g.minv, binary
    s = np.float32(min(BW / g.W, BH / g.H))                # one factor for both axes: ties in x+y and y-x survive the scaling
    return frame, (g.corners * s).astype(np.float32), None, binary


def _batch(n):
    cases = [_batch_case(i) for i in range(n)]
    corners = np.stack([c[1] if c[1] is not None else R.BY_NAME["rot_10"].corners for c in cases])
    minv, ok = Context.corners_to_minv_batch(corners, 450)
    for f, c in enumerate(cases):
        if c[2] is not None:
            minv[f] = c[2]
        elif not ok[f]:
            assert (minv[f] == np.eye(3)).all()            # a degenerate quad: the identity, as the pipeline launches it
    frames = np.stack([c[0] for c in cases])
    binary = np.stack([c[3] for c in cases])
    return frames, minv, binary


@functools.lru_cache(maxsize=None)
def _ref_cells(i, minv_bytes):
    return R.cells(_batch_case(i)[0], np.frombuffer(minv_bytes, np.float64).reshape(3, 3))


@functools.lru_cache(maxsize=None)
def _ref_bands(i, minv_bytes):
    return R.band_counts(_batch_case(i)[3], np.frombuffer(minv_bytes, np.float64).reshape(3, 3))


@pytest.mark.parametrize("n", [1, 7, 83])
def test_warp_cells_fused_and_coverage_batches(ctx, n):
    frames, minv, binary = _batch(n)
    fd, md = _dev(frames), _dev(minv)
    cells = ctx.warp_cells(fd, md).cpu().numpy()
    fbin, fcells = ctx.preprocess_and_warp_cells(fd, md)
    fcells = fcells.cpu().numpy()
    assert torch.equal(fbin, ctx.preprocess(fd))
    bd = _dev(binary)
    cov = ctx.grid_line_coverage(bd, md).cpu().numpy()
    bits = np.packbits(binary > 0, axis=-1, bitorder="little").view("<u4").view(np.int32)
    cov_bits = ctx.grid_line_coverage(_dev(bits), md).cpu().numpy()
    for f in range(n):
        key = minv[f].tobytes()
        want = _ref_cells(f, key)
        _same(cells[f], want, f"warp_cells n={n} frame {f}")
        _same(fcells[f], want, f"fused n={n} frame {f}")
        bands = _ref_bands(f, key)
        _same(cov[f], bands.astype(cov.dtype), f"coverage u8 n={n} frame {f}")
        _same(cov_bits[f], bands.astype(cov.dtype), f"coverage bits n={n} frame {f}")


@pytest.mark.parametrize("row_pad,frame_gap", [(64, 4096), (12, 0), (7, 333)])
def test_padded_rows_and_frame_gaps_hard_geometries(ctx, row_pad, frame_gap):
    """Frames inside a larger buffer (garbage in the padding) give the same cells as warp_ref, for warp_cells and, where its
    4-byte layout rule allows, the fused launch."""
    n = 7
    frames, minv, _ = _batch(n)
    pitch = 3 * BW + row_pad
    fstride = pitch * BH + frame_gap
    buf = torch.randint(0, 256, (n * fstride + 64,), dtype=torch.uint8, device="cuda")
    view = torch.as_strided(buf, (n, BH, BW, 3), (fstride, pitch, 3, 1))
    view.copy_(_dev(frames))
    md = _dev(minv)
    cells = ctx.warp_cells(view, md).cpu().numpy()
    fused = None
    if pitch % 4 == 0 and fstride % 4 == 0:
        fbin, fused = ctx.preprocess_and_warp_cells(view, md)
        fused = fused.cpu().numpy()
        assert torch.equal(fbin, ctx.preprocess(_dev(frames)))
    for f in range(n):
        want = _ref_cells(f, minv[f].tobytes())
        _same(cells[f], want, f"warp_cells pad={row_pad} gap={frame_gap} frame {f}")
        if fused is not None:
            _same(fused[f], want, f"fused pad={row_pad} gap={frame_gap} frame {f}")


# ---- resize --------------------------------------------------------------------------------------------------------------------
RESIZE = [((56, 56), (28, 28)), ((28, 28), (56, 56)), ((40, 40), (28, 28)), ((1, 1), (28, 28)), ((28, 28), (1, 1)),
          ((3, 3), (1000, 1000)), ((37, 90), (28, 45)), ((5, 300), (17, 7)), ((40, 40), (40, 40))]


@pytest.mark.parametrize("src,dst", RESIZE, ids=lambda v: "x".join(map(str, v)))
def test_resize_linear(ctx, src, dst):
    img = np.random.RandomState(src[0] * 7 + dst[1]).randint(0, 256, src, dtype=np.uint8)
    _same(ctx.resize_linear(_dev(img), (dst[1], dst[0])), R.resize(img, (dst[1], dst[0])), f"resize {src}->{dst}")


# ---- views: each equals the same data made contiguous -----------------------------------------------------------------------------
def test_warp_perspective_of_views(ctx):
    rs = np.random.RandomState(21)
    frames = _dev(rs.randint(0, 256, (2, 300, 640, 3), dtype=np.uint8))
    corners = np.array([[30, 20], [290, 35], [300, 280], [15, 260]], np.float32)
    M = Context.corners_to_minv(corners[None], 300)[0]
    md = _dev(M)
    half = frames[0, :, :320]
    assert not half.is_contiguous()
    want = ctx.warp_perspective(half.contiguous(), md, 300)
    _same(want, R.warp(half.cpu().numpy(), M, 300), "contiguous half frame")
    _same(ctx.warp_perspective(half, md, 300), want.cpu().numpy(), "frames[0, :, :W//2]")
    gray = ctx.gray(frames)[1]
    crop = gray[10:290, 30:330]
    _same(ctx.warp_perspective(crop, md, 300), ctx.warp_perspective(crop.contiguous(), md, 300).cpu().numpy(), "gray crop")
    _same(ctx.warp_perspective(crop, md, 300), R.warp(crop.cpu().numpy(), M, 300), "gray crop vs warp_ref")
    tr = gray[:, :300].t()
    _same(ctx.warp_perspective(tr, md, 300), ctx.warp_perspective(tr.contiguous(), md, 300).cpu().numpy(), "transposed gray")


def test_extract_cells_and_resize_of_views(ctx):
    rs = np.random.RandomState(22)
    big = _dev(rs.randint(0, 256, (500, 530, 3), dtype=np.uint8))
    for grid in (big[:450, :450], big[20:470, 40:490], big[:450, :450, 1]):
        assert not grid.is_contiguous()
        _same(ctx.extract_cells(grid, 28, 5, 5), ctx.extract_cells(grid.contiguous(), 28, 5, 5).cpu().numpy(), f"extract {grid.shape}")
        _same(ctx.extract_cells(grid, 28, 5, 5), R.extract(grid.cpu().numpy(), 28, 0.1), f"extract {grid.shape} vs warp_ref")
    img = big[:, :, 2]
    for view, dsize in ((img[5:45, 7:47], (28, 28)), (img[100:103, 9:12], (1000, 1000)), (img[3:59, 60:116], (28, 28))):
        _same(ctx.resize_linear(view, dsize), ctx.resize_linear(view.contiguous(), dsize).cpu().numpy(), f"resize {view.shape}")
        _same(ctx.resize_linear(view, dsize), R.resize(view.cpu().numpy(), dsize), f"resize {view.shape} vs warp_ref")


def test_cell_methods_of_cropped_views(ctx):
    rs = np.random.RandomState(23)
    big = _dev(rs.randint(0, 256, (37, 32, 32), dtype=np.uint8))
    cells = big[:, 2:30, 2:30]
    assert not cells.is_contiguous()
    dense = cells.contiguous()
    r1, t1 = ctx.cell_ink_ratio(cells)
    r2, t2 = ctx.cell_ink_ratio(dense)
    assert torch.equal(r1, r2) and torch.equal(t1, t2)
    assert torch.equal(ctx.preprocess_cells(cells), ctx.preprocess_cells(dense))
    ctx.load_state_dict(cnn_oracle.random_state_dict(77))
    for glue in (Context.GLUE_NORMALIZE, Context.GLUE_RUNPY):
        assert torch.equal(ctx.cnn_forward(cells, glue=glue), ctx.cnn_forward(dense, glue=glue)), glue
