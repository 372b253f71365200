"""cv/grid_v2.py on the GPU against tests/grid_v2_ref.py: the Harris response and corner list and the affine warp of
csrc/k13_grid_v2.hip bit for bit -- on plain frames first, then on inputs built for the branches those do not reach (last tiles a
pixel wide, thresholds that tie, more than 2048 candidates, frames at the size limit, every bilinear fraction, rounding ties,
degenerate matrices) --, detect_grid end to end on small synthetic frames that reach each of its methods, and the grid="v2" hook
of the pipeline."""
import os

import numpy as np
import pytest
import torch

import grid_v2_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module():
    import sudoku_vision_amd.cv.grid_v2 as m
    return m


def _noise(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_harris(ctx, img, **kw):
    want, resp, ncand = R.harris_corners(img, **kw)
    got, got_resp = ctx.harris_corners(img, want_response=True, **kw)
    assert got_resp.dtype == np.float32 and got_resp.shape == img.shape
    bad = np.argwhere(_bits(got_resp) != _bits(resp))
    assert bad.size == 0, f"response: {len(bad)} pixels differ, first at {bad[0].tolist()}"
    assert got.dtype == np.float32 and got.shape == want.shape and (got == want).all(), (got, want)
    return want, ncand


# ---- Harris ---------------------------------------------------------------------------------------------------------------
def test_harris_noise_not_a_tile_multiple(ctx):
    want, ncand = _check_harris(ctx, _noise((37, 53), 1), max_corners=100, quality_level=0.01, min_distance=3)
    assert 4 < len(want) < ncand                             # the distance rule removed some


def test_harris_more_than_one_tile_each_way(ctx):
    _check_harris(ctx, _noise((40, 150), 2), max_corners=60, quality_level=0.05, min_distance=6)


def test_harris_batch_padded_layout_with_a_constant_frame(ctx):
    frames = np.stack([_noise((64, 96), 3), np.full((64, 96), 77, np.uint8), _noise((64, 96), 4)])
    buf = torch.full((3, 64 + 5, 96 + 32), 255, dtype=torch.uint8, device=ctx.device)
    view = buf[:, :64, :96]
    view.copy_(torch.from_numpy(frames))
    assert view.stride(1) > 96 and view.stride(0) > 64 * view.stride(1)
    corners, counts, resp = ctx.harris_corners(view, max_corners=50, min_distance=5, want_response=True)
    assert isinstance(corners, torch.Tensor) and corners.shape == (3, 50, 2) and counts.dtype == torch.int32
    for f in range(3):
        want, want_resp, _ = R.harris_corners(frames[f], max_corners=50, min_distance=5)
        assert (_bits(resp[f].cpu().numpy()) == _bits(want_resp)).all()
        assert int(counts[f]) == len(want) and (corners[f, :len(want)].cpu().numpy() == want).all()
    assert int(counts[1]) == 0 and int(counts[0]) > 0 and int(counts[2]) > 0
    single = ctx.harris_corners(frames[2], max_corners=50, min_distance=5)                       # the same frame alone
    assert (single == corners[2, :int(counts[2])].cpu().numpy()).all()


def test_harris_checkerboard_ties_distance_and_cap(ctx):
    yy, xx = np.mgrid[0:96, 0:96]
    board = (((yy // 8) + (xx // 8)) % 2 * 255).astype(np.uint8)
    resp = R.harris_response(board)
    cand = R.harris_candidates(resp, 0.01)
    values = [c[0] for c in cand]
    assert len(cand) > 50 and len(set(values)) < len(values) / 4            # many exactly equal responses: raster order decides
    far, _ = _check_harris(ctx, board, max_corners=100, quality_level=0.01, min_distance=10)
    near, _ = _check_harris(ctx, board, max_corners=100, quality_level=0.01, min_distance=1)
    assert len(far) < len(near)                                              # neighbouring candidates fell to the distance rule
    capped, _ = _check_harris(ctx, board, max_corners=5, quality_level=0.01, min_distance=10)
    assert len(capped) == 5 and (capped == far[:5]).all()


def test_harris_smallest_frame_and_too_small(ctx):
    import sudoku_vision_amd as sva
    tiny = np.array([[0, 0, 0], [0, 255, 10], [0, 30, 0]], np.uint8)
    _check_harris(ctx, tiny, max_corners=10, quality_level=0.01, min_distance=1)
    _check_harris(ctx, _noise((3, 70), 6), max_corners=10, quality_level=0.01, min_distance=1)
    with pytest.raises(sva._native.NativeError, match="SV_ERR_BAD_ARG"):
        ctx.harris_corners(np.zeros((2, 5), np.uint8))


def test_harris_candidate_overflow_is_an_error(ctx):
    import sudoku_vision_amd as sva
    img = _noise((37, 53), 1)
    _, _, ncand = R.harris_corners(img, min_distance=3)
    assert ncand > 8
    with pytest.raises(sva._native.NativeError, match="SV_ERR_BUFFER"):
        ctx.harris_corners(img, min_distance=3, cand_capacity=ncand - 1)
    got = ctx.harris_corners(img, min_distance=3, cand_capacity=ncand)       # exactly enough
    assert (got == R.harris_corners(img, min_distance=3)[0]).all()


# ---- warpAffine -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("angle", [7.3, -38.0])
@pytest.mark.parametrize("border", [255, 0])
def test_warp_affine_rotation_into_the_enlarged_box(ctx, angle, border):
    img = _noise((45, 70), 8)
    want, matrix = R.rotate_image(img, angle, border_value=border)
    got = ctx.warp_affine(img, matrix, (want.shape[1], want.shape[0]), border)
    assert got.dtype == np.uint8 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} pixels differ, first at {bad[0].tolist()}"
    assert (want == border).any() and (want != border).any()
    if border == 255:                                        # the drop-in's rotate_image is this call
        rotated, m2 = _module().rotate_image(img, angle)
        assert (m2 == matrix).all() and (rotated == want).all()


def test_warp_affine_identity_and_batch(ctx):
    img = _noise((45, 70), 9)
    eye = np.array([[1, 0, 0], [0, 1, 0]], np.float64)
    assert (ctx.warp_affine(img, eye, (70, 45), 0) == img).all()
    assert (R.warp_affine(img, eye, (70, 45), 0) == img).all()
    pair = np.stack([img, _noise((45, 70), 10)])
    mats = np.stack([R.rotation_matrix((35, 22), 12.5, 1.0), np.array([[0.9, 0.2, -3.5], [-0.15, 1.1, 4.25]])])
    got = ctx.warp_affine(torch.from_numpy(pair).to(ctx.device), mats, (81, 52), 17)
    assert isinstance(got, torch.Tensor) and got.shape == (2, 52, 81)
    for f in range(2):
        assert (got[f].cpu().numpy() == R.warp_affine(pair[f], mats[f], (81, 52), 17)).all()


# ---- Harris where the frames above do not reach ----------------------------------------------------------------------------
# The inputs come from grid_v2_ref.py; tests/test_grid_v2_ref.py asserts on the CPU what each one does to the restatement (which
# branch of the kernels it is built for), so that a weak input fails there and not silently here.
@pytest.mark.parametrize("shape", R.TILING_SHAPES)
def test_harris_last_tile_one_or_two_pixels(ctx, shape):
    _check_harris(ctx, R.noise(shape, 5), max_corners=200, quality_level=0.01, min_distance=2)
    inset, _ = _check_harris(ctx, R.corner_squares(shape), max_corners=10, quality_level=0.01, min_distance=3)
    assert len(inset) == 4
    flush, _ = _check_harris(ctx, R.corner_squares(shape, inset=0), max_corners=10, quality_level=0.01, min_distance=3)
    assert len(flush) == 0


def test_harris_frame_maximum_on_the_border(ctx):
    img = R.border_maximum_frame()
    one, ncand = _check_harris(ctx, img, max_corners=10, quality_level=0.01, min_distance=1)
    assert ncand == 1 and one.tolist() == [[15, 11]]
    assert (ctx.harris_corners(img, max_corners=10, min_distance=1, cand_capacity=1) == one).all()       # P = 1: the sort does not run
    none, ncand = _check_harris(ctx, img, max_corners=10, quality_level=1.0, min_distance=1)
    assert ncand == 0 and len(none) == 0                     # the only value that reaches the maximum lies on the excluded frame


@pytest.mark.parametrize("quality", [1.0, 0.0])
@pytest.mark.parametrize("max_corners,min_distance", [(100, 10), (4096, 0), (4096, 1)])
def test_harris_checkerboard_at_both_ends_of_quality(ctx, quality, max_corners, min_distance):
    want, ncand = _check_harris(ctx, R.checkerboard(), max_corners=max_corners, quality_level=quality, min_distance=min_distance)
    assert ncand == 484 and (len(want) == 484 or min_distance == 10)          # v == quality * max is kept


@pytest.mark.parametrize("min_distance", [0, 3])
def test_harris_quality_zero_orders_tiny_responses(ctx, min_distance):
    _, ncand = _check_harris(ctx, R.wide_range_noise(), max_corners=4096, quality_level=0.0, min_distance=min_distance)
    assert ncand > 100


@pytest.mark.parametrize("k", [0.25, 0.0])
def test_harris_k_extremes(ctx, k):
    want, ncand = _check_harris(ctx, _noise((37, 53), 1), max_corners=100, quality_level=0.01, min_distance=3, k=k)
    assert (ncand == 0 and len(want) == 0) if k else ncand > 50              # k = 0.25: the maximum is negative, no corner in a frame that is not flat


@pytest.mark.parametrize("min_distance", [2, 0, 5])
def test_harris_more_than_2048_candidates(ctx, min_distance):
    want, ncand = _check_harris(ctx, R.noise(*R.MANY), max_corners=4096, quality_level=0.01, min_distance=min_distance)
    assert 2048 < ncand <= 4096 and (len(want) == ncand if min_distance < 5 else 1024 < len(want) < ncand)     # at 5 the rule drops hundreds


def test_harris_power_of_two_candidates_in_exactly_that_capacity(ctx):
    import sudoku_vision_amd as sva
    img = R.noise(*R.POWER_OF_TWO)
    want, ncand = _check_harris(ctx, img, max_corners=100, quality_level=0.01, min_distance=3)
    assert ncand == 64
    assert (ctx.harris_corners(img, max_corners=100, min_distance=3, cand_capacity=64) == want).all()
    with pytest.raises(sva._native.NativeError, match="SV_ERR_BUFFER"):
        ctx.harris_corners(img, max_corners=100, min_distance=3, cand_capacity=63)


def test_harris_max_corners_caps(ctx):
    img = R.noise(*R.OVER_CAP)
    full, ncand = _check_harris(ctx, img, max_corners=4096, quality_level=0.01, min_distance=0)          # SV_HARRIS_MAX_CORNERS
    assert ncand > 4096 and len(full) == 4096
    one, _ = _check_harris(ctx, img, max_corners=1, quality_level=0.01, min_distance=0)
    assert one.tolist() == full[:1].tolist()
    import sudoku_vision_amd as sva
    with pytest.raises(sva._native.NativeError, match="SV_ERR_BAD_ARG"):
        ctx.harris_corners(img, max_corners=4097)


def test_harris_batch_of_uneven_candidate_counts(ctx):
    frames = R.uneven_batch()
    kw = dict(max_corners=4096, quality_level=0.01, min_distance=2)
    corners, counts, resp = ctx.harris_corners(frames, want_response=True, **kw)
    assert corners.shape == (3, 4096, 2) and counts.shape == (3,)
    sizes = []
    for f in range(3):
        want, want_resp, ncand = R.harris_corners(frames[f], **kw)
        sizes.append(ncand)
        assert (_bits(resp[f]) == _bits(want_resp)).all()
        assert int(counts[f]) == len(want) and (corners[f, :len(want)] == want).all()
        assert (ctx.harris_corners(frames[f], **kw) == want).all()                                   # the same frame alone
    assert sizes[0] > 10 * sizes[1] and sizes[1] > 10 * sizes[2] > 0


@pytest.mark.parametrize("squares", [R.TALL_SQUARES, R.TALL_PAIR], ids=["65536 rows apart", "a pair beyond row 65536"])
def test_harris_refuses_rows_beyond_16_bits(ctx, squares):
    """k_harris_select keeps a corner as x | y << 16; the entry takes no frame in which that could alias (test_grid_v2_ref.py has the
    lists a wider kernel would have to give)."""
    import sudoku_vision_amd as sva
    with pytest.raises(sva._native.NativeError, match="SV_ERR_BAD_ARG: sv_harris_corners_u8: bad shape"):
        ctx.harris_corners(R.square_column(R.TALL, squares), quality_level=0.01, min_distance=8)
    with pytest.raises(sva._native.NativeError, match="SV_ERR_BAD_ARG: sv_harris_corners_u8: W must be below 65536"):
        ctx.harris_corners(np.ascontiguousarray(R.square_column(R.TALL, squares).T), quality_level=0.01, min_distance=8)


def test_harris_tallest_and_widest_frame(ctx):
    img = R.square_column(R.LIMIT, R.LIMIT_SQUARES)
    want, ncand = _check_harris(ctx, img, max_corners=100, quality_level=0.01, min_distance=8)
    assert ncand == 12 and want.tolist() == [[2, 65519], [2, 32761], [2, 32769], [2, 9], [2, 29999]]
    wide, ncand = _check_harris(ctx, np.ascontiguousarray(img.T), max_corners=100, quality_level=0.01, min_distance=8)
    assert ncand == 12 and len(wide) == 5 and wide[0, 0] > 65500


# ---- warpAffine where the rotations above do not reach ----------------------------------------------------------------------
def _check_warp(ctx, src, matrix, dsize, border):
    want = R.warp_affine(src, matrix, dsize, border)
    got = ctx.warp_affine(src, np.asarray(matrix, np.float64), dsize, border)
    assert got.dtype == np.uint8 and got.shape == want.shape == (dsize[1], dsize[0])
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} pixels differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    return want


@pytest.mark.parametrize("border", [0, 255, 128])
@pytest.mark.parametrize("source", list(R.FRACTION_SOURCES))
def test_warp_affine_every_fraction_pair_inside_and_at_each_border(ctx, source, border):
    _check_warp(ctx, R.FRACTION_SOURCES[source], R.fraction_sweep_matrix(), R.FRACTION_DSIZE, border)


@pytest.mark.parametrize("case", list(R.tie_cases()))
@pytest.mark.parametrize("border", [0, 128])
def test_warp_affine_ties_round_half_to_even(ctx, case, border):
    src, matrix, shows = R.tie_cases()[case]
    want = _check_warp(ctx, src, matrix, R.TIE_DSIZE, border)
    for rounding in ("half_away", "truncate"):
        if shows in (rounding, "both"):
            assert (R.warp_affine(src, matrix, R.TIE_DSIZE, border, rounding=rounding) != want).sum() >= 8


@pytest.mark.parametrize("case", list(R.DEGENERATE_MATRICES))
def test_warp_affine_degenerate_matrices(ctx, case):
    src = R.noise((9, 13), 3)
    want = _check_warp(ctx, src, R.DEGENERATE_MATRICES[case], (17, 6), 77)
    if case == "singular":
        assert (want == src[0, 0]).all()
    if case == "far":
        assert (want == 77).all()


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1)])
def test_warp_affine_sources_with_no_inside(ctx, shape):
    src = R.noise(shape, 4)
    want = _check_warp(ctx, src, [[1.3, 0.2, 1.7], [-0.1, 1.6, 2.2]], (16, 12), 200)
    assert (want == 200).any() and (want != 200).any()
    _check_warp(ctx, src, [[1, 0, 0], [0, 1, 0]], (shape[1] + 1, shape[0] + 1), 9)


@pytest.mark.parametrize("dsize", [(1, 1), (65, 5)])
def test_warp_affine_destination_sizes(ctx, dsize):
    want = _check_warp(ctx, _noise((45, 70), 8), R.rotation_matrix((10, 3), -21.0, 0.8), dsize, 31)
    assert dsize == (1, 1) or ((want == 31).any() and (want != 31).any())


def test_warp_affine_gapped_batch_one_matrix_per_frame(ctx):
    """Padded rows, gaps between the frames and an odd base address (test_gpu_preprocess_v2._gapped's layout) over a buffer of 0xA5."""
    n, H, W = 3, 23, 37
    imgs = np.stack([_noise((H, W), 20 + i) for i in range(n)])
    pitch, offset = W + 5, 1
    fstride = pitch * H + 13
    buf = torch.full((offset + n * fstride + 64,), 0xA5, dtype=torch.uint8, device=ctx.device)
    view = buf[offset:].as_strided((n, H, W), (fstride, pitch, 1))
    view.copy_(torch.from_numpy(imgs).to(ctx.device))
    assert view.data_ptr() % 2 == 1 and not view.is_contiguous()
    mats = np.stack([R.rotation_matrix((18, 11), 33.0, 1.1), np.array([[0.7, -0.3, 6.5], [0.25, 1.2, -2.75]]), np.array([[-1, 0, W - 0.5], [0, 1, 0.25]])])
    got = ctx.warp_affine(view, mats, (41, 29), 0x5A)
    assert isinstance(got, torch.Tensor) and got.shape == (n, 29, 41)
    for f in range(n):
        want = R.warp_affine(imgs[f], mats[f], (41, 29), 0x5A)
        assert (got[f].cpu().numpy() == want).all(), f
        assert (want == 0x5A).any() and (want != 0x5A).any() and not (want == 0xA5).all()


# ---- detect_grid end to end -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    """240x320 synthetic frames (integer noise: the same on every machine) -> {name: (binary, gray)} with K1's binary from the oracle.
    notched: the outer border erased around the four corners, so the outline is no quadrilateral but the lines remain."""
    import sv_oracle as o
    from sudoku_vision_amd.synth import synth_frames
    frames, corners, _ = synth_frames(1, 240, 320, seed=7, device="cpu", noise="int")
    frame, quad = frames[0].numpy(), corners[0]
    paper = frame[2, 2].copy()

    def notched(cells):
        g = frame.copy()
        for i in range(4):
            r = int(np.linalg.norm(quad[(i + 1) % 4] - quad[i]) / 9 * cells)
            x, y = int(quad[i][0]), int(quad[i][1])
            g[max(y - r, 0):y + r, max(x - r, 0):x + r] = paper
        return g

    def rotated(g, angle):
        return np.stack([R.rotate_image(g[:, :, c], angle, border_value=int(paper[c]))[0] for c in range(3)], -1)

    blank = np.empty_like(frame)
    blank[:] = paper
    imgs = {"clean": frame, "broken": notched(0.6), "broken_rotated": rotated(notched(0.6), 12.0), "corners_only": rotated(notched(1.2), 12.0), "blank": blank}
    return {k: (o.preprocess_for_grid_detection(v), o.gray(v)) for k, v in imgs.items()}


def _same_detection(got, want):
    assert got.method == want["method"] and got.confidence == want["confidence"] and got.rotation_angle == want["rotation_angle"]
    assert got.is_partial is False and got.debug_info == want["debug_info"]
    if want["corners"] is None:
        assert got.corners is None
    else:
        assert got.corners.dtype == np.float32 and got.corners.shape == (4, 2) and (got.corners == want["corners"]).all(), (got.corners, want["corners"])


@pytest.mark.parametrize("name,method", [("clean", "contour"), ("broken", "lines"), ("broken_rotated", "contour_rotated"), ("corners_only", "harris_ransac"),
                                         ("blank", "none")])
def test_detect_grid_methods(ctx, scenes, name, method):
    binary, gray = scenes[name]
    # the design of the input, on the CPU: which methods of the restatement fail and which one succeeds
    if method != "contour":
        assert R.detect_grid_contour(binary) is None
    if method == "lines":
        assert R.detect_grid_lines(binary) is not None
    np.random.seed(0)
    want = R.detect_grid(binary, gray)
    assert want["method"] == method
    np.random.seed(0)
    got = _module().detect_grid(binary, gray)
    _same_detection(got, want)
    if method == "contour_rotated":
        assert abs(abs(got.rotation_angle) - 12) < 1 and set(got.debug_info) == {"detected_rotation"}
    if method == "harris_ransac":
        assert got.debug_info["harris_corners"] >= 4 and set(got.debug_info) == {"detected_rotation", "harris_corners"}
    if method == "none":
        assert got.debug_info["harris_corners"] == 0 and got.corners is None and got.confidence == 0
        assert _module().detect_grid(binary, gray, try_multiple_methods=False).debug_info == {}


def test_detect_grid_takes_tensors(ctx, scenes):
    binary, gray = scenes["broken_rotated"]
    want = _module().detect_grid(binary, gray)
    got = _module().detect_grid(torch.from_numpy(binary).to(ctx.device), torch.from_numpy(gray).to(ctx.device))
    assert got.method == want.method == "contour_rotated" and (got.corners == want.corners).all()


# ---- the pipeline hook ----------------------------------------------------------------------------------------------------
def test_recognize_image_grid_v2(ctx, golden_dir):
    import cnn_oracle
    import sudoku_vision_amd as sva
    from sudoku_vision_amd import imgcodecs
    from sudoku_vision_amd.pipeline import recognize_image
    sd = cnn_oracle.random_state_dict(1234)
    img = imgcodecs.imread(os.path.join(golden_dir, "sample_1.jpg"), device=True, ctx=ctx, reduce=4)
    binary = ctx.preprocess(img[None])[0]
    v1 = recognize_image(img, sd, ctx=ctx)
    explicit = recognize_image(img, sd, ctx=ctx, grid="v1")
    assert v1 is not None and set(v1) == set(explicit) == {"grid", "digits", "confidence", "logits", "corners"}
    assert (v1["corners"] == sva.host.find_grid_corners(binary.cpu().numpy())).all()             # the default path: v1's search, untouched
    assert all((v1[k] == explicit[k]).all() for k in ("digits", "confidence", "logits", "corners"))
    v2 = recognize_image(img, sd, ctx=ctx, grid="v2")
    det = _module().detect_grid(binary, ctx.gray(img[None])[0])
    assert v2 is not None and det.corners is not None
    assert v2["detection_method"] == det.method and v2["detection_confidence"] == det.confidence and v2["rotation_angle"] == det.rotation_angle
    assert (v2["corners"] == det.corners).all() and v2["digits"].shape == (81,)
    with pytest.raises(ValueError):
        recognize_image(img, sd, ctx=ctx, grid="v3")


def test_run_pipeline_grid_v2_and_module_warp(ctx, golden_dir):
    import cnn_oracle
    from sudoku_vision_amd import imgcodecs
    from sudoku_vision_amd.pipeline import recognize_image, run_pipeline
    sd = cnn_oracle.random_state_dict(1234)
    path = os.path.join(golden_dir, "sample_1.jpg")
    res = run_pipeline(path, sd, ctx=ctx, reduce=4, grid="v2")
    img = imgcodecs.imread(path, device=True, ctx=ctx, reduce=4)
    rec = recognize_image(img, sd, ctx=ctx, grid="v2")
    assert res.error is None or not res.error.startswith("Grid detection"), res.error
    assert (res.detection_method, res.detection_confidence, res.rotation_angle) == (rec["detection_method"], rec["detection_confidence"], rec["rotation_angle"])
    assert [p.digit for p in res.predictions] == [int(d) for d in rec["digits"]]
    base = run_pipeline(path, sd, ctx=ctx, reduce=4)
    assert not hasattr(base, "detection_method") and base.recognized_grid == run_pipeline(path, sd, ctx=ctx, reduce=4, grid="v1").recognized_grid
    # the module's warp_perspective is K2's warp of the ordered corners, for arrays and tensors
    m = _module()
    minv = ctx.minv_to_device(type(ctx).corners_to_minv(m.order_points(rec["corners"])[None], 450))
    want = ctx.warp_perspective(img, minv, 450).cpu().numpy()
    assert (res.warped_grid == want).all()
    assert (m.warp_perspective(img, rec["corners"][::-1].copy()).cpu().numpy() == want).all()      # any corner order
    assert (m.warp_perspective(img.cpu().numpy(), rec["corners"]) == want).all()
    small = m.warp_perspective(img[:, :, 0].contiguous(), rec["corners"], output_size=90)
    assert small.shape == (90, 90) and small.dtype == torch.uint8
