"""GPU (-m gpu): the HIP path, called through the C ABI, against the CPU oracle on the same seeded
inputs.  Integer/byte stages: bit-exact.  CNN logits: |diff| <= 1e-4 (fp32, north_star tolerance);
digit indices equal."""
import os

import numpy as np
import pytest
import torch

import cnn_oracle
import sv_oracle as o

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4


def _frames(n, H, W, seed):
    from sudoku_vision_amd.synth import synth_frames
    return synth_frames(n, H, W, seed=seed, device="cuda")


@pytest.mark.parametrize("H,W", [(270, 480), (97, 131), (1080, 1920)])
def test_preprocess_fused_bit_exact(ctx, H, W):
    frames, _, _ = _frames(2, H, W, seed=H)
    got = ctx.preprocess(frames).cpu().numpy()
    host = frames.cpu().numpy()
    for i in range(2):
        assert (got[i] == o.preprocess_for_grid_detection(host[i])).all()


def test_preprocess_random_noise_bit_exact(ctx):
    """Pure noise maximises the number of near-tie means and exercises every border path."""
    rs = np.random.RandomState(5)
    img = rs.randint(0, 256, (3, 75, 140, 3)).astype(np.uint8)
    got = ctx.preprocess(torch.from_numpy(img).cuda()).cpu().numpy()
    for i in range(3):
        assert (got[i] == o.preprocess_for_grid_detection(img[i])).all()


def test_standalone_stages_bit_exact(ctx):
    rs = np.random.RandomState(6)
    bgr = rs.randint(0, 256, (2, 61, 83, 3)).astype(np.uint8)
    d = torch.from_numpy(bgr).cuda()
    g = ctx.gray(d)
    assert (g.cpu().numpy() == np.stack([o.gray(b) for b in bgr])).all()
    for k in (1, 3, 5, 7):
        assert (ctx.blur(g, k).cpu().numpy() == np.stack([o.gaussian_blur(x, k) for x in g.cpu().numpy()])).all()
    for block, c, inv in ((3, 2, True), (5, 0, False), (11, 2, True), (11, 2, False), (15, 3.5, True), (31, -1, False)):
        got = ctx.adaptive_threshold(g, block, c, inv).cpu().numpy()
        exp = np.stack([o.adaptive_threshold(x, block, c, inv) for x in g.cpu().numpy()])
        assert (got == exp).all(), (block, c, inv)


def test_fused_equals_staged(ctx):
    frames, _, _ = _frames(1, 200, 300, seed=9)
    a = ctx.preprocess(frames)
    b = ctx.adaptive_threshold(ctx.blur(ctx.gray(frames), 5), 11, 2, True)
    assert torch.equal(a, b)


@pytest.mark.parametrize("H,W", [(270, 480), (1080, 1920)])
def test_warp_cells_bit_exact(ctx, H, W):
    import sudoku_vision_amd as sva
    frames, corners, _ = _frames(3, H, W, seed=W)
    minv = ctx.minv_to_device(sva.Context.corners_to_minv(corners))
    got = ctx.warp_cells(frames, minv).cpu().numpy()
    host = frames.cpu().numpy()
    for i in range(3):
        assert (got[i] == o.warp_cells(host[i], corners[i])).all()


def test_warp_perspective_and_extract_bit_exact(ctx):
    import sudoku_vision_amd as sva
    frames, corners, _ = _frames(1, 540, 960, seed=2)
    host = frames[0].cpu().numpy()
    # corners partly outside the frame: constant-0 border taps
    c2 = corners[0].copy()
    c2[0] = [-40, -25]
    for cs, S, inset in ((corners[0], 450, 0.0), (c2, 450, 0.0), (corners[0], 300, 0.0)):
        minv = ctx.minv_to_device(sva.Context.corners_to_minv(cs[None], S, inset))
        w = ctx.warp_perspective(frames[0], minv, S)
        exp = o.warp_perspective(host, cs, S, inset)
        assert (w.cpu().numpy() == exp).all()
        for cell_size, margin in ((28, 0.1), (32, 0.2), (28, 0.0)):
            mh = int((S // 9) * margin)
            cells = ctx.extract_cells(w, cell_size, mh, mh).cpu().numpy()
            assert (cells == o.extract_cells(exp, cell_size, margin)).all()
    # gray input
    g = ctx.gray(frames)[0]
    minv = ctx.minv_to_device(sva.Context.corners_to_minv(corners[:1]))
    wg = ctx.warp_perspective(g, minv, 450)
    assert (wg.cpu().numpy() == o.warp_perspective(g.cpu().numpy(), corners[0])).all()
    assert (ctx.extract_cells(wg, 28, 5, 5).cpu().numpy() == o.extract_cells(wg.cpu().numpy())).all()


def _check_cnn(ctx, sd, x, want_digits=True):
    ctx.load_state_dict(sd)
    logits, digits, conf = ctx.cnn_forward(torch.from_numpy(x).cuda(), want_digits=True)
    el, ed, ec = cnn_oracle.predict(sd, x if x.dtype != np.uint8 else o.cells_to_input(x)[:, None])
    diff = np.abs(logits.cpu().numpy() - el.numpy()).max()
    assert diff <= LOGIT_TOL, diff
    top2 = np.sort(el.numpy(), 1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2 * LOGIT_TOL          # argmax is only defined up to the logit tolerance
    assert (digits.cpu().numpy()[clear] == ed.numpy()[clear]).all()
    assert np.abs(conf.cpu().numpy() - ec.numpy()).max() <= 1e-5
    return logits, digits


@pytest.mark.parametrize("B", [1, 2, 3, 81, 200])
def test_cnn_random_weights(ctx, B):
    sd = cnn_oracle.random_state_dict(1234)
    _check_cnn(ctx, sd, cnn_oracle.golden_inputs(B + 7, B))


def test_cnn_golden_fixtures(ctx, golden_dir):
    g = np.load(os.path.join(golden_dir, "cnn_random_seed1234.npz"))
    sd = cnn_oracle.random_state_dict(int(g["seed"]))
    logits, digits = _check_cnn(ctx, sd, cnn_oracle.golden_inputs(int(g["x_seed"]), 81))
    assert np.abs(logits.cpu().numpy() - g["logits"]).max() <= LOGIT_TOL
    g2 = np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz"))
    sd2 = {k: torch.from_numpy(g2[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS}
    logits, digits = _check_cnn(ctx, sd2, cnn_oracle.golden_inputs(int(g2["x_seed"]), 162))
    assert np.abs(logits.cpu().numpy() - g2["logits"]).max() <= LOGIT_TOL
    assert (digits.cpu().numpy() == g2["digits"]).all()          # trained weights: bit-exact digit indices


def test_cnn_u8_cells_entry(ctx):
    sd = cnn_oracle.random_state_dict(3)
    cells = np.random.RandomState(8).randint(0, 256, (100, 28, 28)).astype(np.uint8)
    logits, _ = _check_cnn(ctx, sd, cells)
    # a cell buffer that is not 4-byte aligned (the stream kernel reads cells as dwords: such a buffer takes the direct kernel)
    buf = torch.zeros(100 * 784 + 8, dtype=torch.uint8, device="cuda")
    for off in (1, 2, 3):
        view = buf[off:off + 100 * 784].view(100, 28, 28)
        view.copy_(torch.from_numpy(cells))
        assert view.data_ptr() % 4 == off
        got = ctx.cnn_forward(view)
        assert (got - logits).abs().max().item() <= 2e-5


def test_digitcnn_module_dropin(ctx, golden_dir):
    """model = DigitCNN().to(device); model.load_state_dict(...); model.eval(); model(x)  (pipeline/run.py:98-143)."""
    from sudoku_vision_amd.ml.model import DigitCNN
    g2 = np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz"))
    sd2 = {k: torch.from_numpy(g2[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS}
    model = DigitCNN().to("cuda")
    model.load_state_dict(sd2)
    model.eval()
    x = torch.from_numpy(cnn_oracle.golden_inputs(int(g2["x_seed"]), 162)).cuda()
    with torch.no_grad():
        out = model(x)
        one = model(x[5:6])
    assert np.abs(out.cpu().numpy() - g2["logits"]).max() <= LOGIT_TOL
    assert np.abs(one.cpu().numpy() - g2["logits"][5:6]).max() <= LOGIT_TOL
    assert (out.argmax(1).cpu().numpy() == g2["digits"]).all()
    with pytest.raises(RuntimeError):
        model(x.cpu())
    model.train()
    with pytest.raises(NotImplementedError):
        model(x)


def test_frames_to_digits_end_to_end(ctx, golden_dir):
    import sudoku_vision_amd as sva
    g2 = np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz"))
    sd = {k: torch.from_numpy(g2[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS}
    frames, corners, _ = _frames(4, 1080, 1920, seed=77)
    ctx.load_state_dict(sd)
    minv = ctx.minv_to_device(sva.Context.corners_to_minv(corners))
    out = ctx.frames_to_digits(frames, minv, keep_cells=True)
    host = frames.cpu().numpy()
    for i in range(4):
        cells = o.warp_cells(host[i], corners[i])
        assert (out["cells"][i].cpu().numpy() == cells).all()
        el, ed, ec = cnn_oracle.predict(sd, o.cells_to_input(cells)[:, None])
        assert np.abs(out["logits"][i].cpu().numpy() - el.numpy()).max() <= LOGIT_TOL
        assert (out["digits"][i].cpu().numpy() == ed.numpy()).all()


def test_dropin_numpy_functions(ctx):
    """numpy in -> numpy out through the reference-named functions, in the reference's call order."""
    from sudoku_vision_amd.cv.preprocess import preprocess_for_grid_detection, grayscale, blur, threshold
    from sudoku_vision_amd.cv.grid import warp_perspective
    from sudoku_vision_amd.cv.extract import extract_cells
    frames, corners, _ = _frames(1, 360, 640, seed=21)
    img = frames[0].cpu().numpy()
    binary = preprocess_for_grid_detection(img)
    assert isinstance(binary, np.ndarray) and binary.dtype == np.uint8 and binary.shape == (360, 640)
    assert (binary == o.preprocess_for_grid_detection(img)).all()
    assert (threshold(blur(grayscale(img), ksize=5), block_size=11, c=2) == binary).all()
    g = grayscale(img)
    assert grayscale(g) is g
    warped = warp_perspective(img, corners[0][[2, 0, 3, 1]].astype(np.int32))      # any corner order, int input
    assert warped.shape == (450, 450, 3) and (warped == o.warp_perspective(img, corners[0])).all()
    cells = extract_cells(warped)
    assert isinstance(cells, list) and len(cells) == 81 and all(c.shape == (28, 28) and c.dtype == np.uint8 for c in cells)
    assert (np.stack(cells) == o.extract_cells(warped)).all()


def test_pipeline_with_host_corner_search(ctx, golden_dir):
    """K1 -> D2H -> host corner search -> K2 -> K3, chunked and double-buffered, against the oracle run end to end."""
    import sudoku_vision_amd as sva
    from sudoku_vision_amd.pipeline import FramePipeline, recognize_image
    g2 = np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz"))
    sd = {k: torch.from_numpy(g2[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS}
    ctx.load_state_dict(sd)
    frames, corners_gt, _ = _frames(7, 540, 960, seed=31)
    frames[3] = 200                                                   # a frame without a grid
    pipe = FramePipeline(ctx, 540, 960, chunk=3, host_threads=2)
    out = pipe.run(frames)
    torch.cuda.synchronize()
    host = frames.cpu().numpy()
    assert out["found"].tolist() == [True, True, True, False, True, True, True]
    for i in range(7):
        if i == 3:
            assert (out["digits"][i].cpu().numpy() == 0).all()
            continue
        c = o.find_grid_contour(o.preprocess_for_grid_detection(host[i]))
        assert (out["corners"][i] == c).all()
        cells = o.warp_cells(host[i], c.astype(np.float32))
        el, ed, ec = cnn_oracle.predict(sd, o.cells_to_input(cells)[:, None])
        assert np.abs(out["logits"][i].cpu().numpy() - el.numpy()).max() <= LOGIT_TOL
        assert (out["digits"][i].cpu().numpy() == ed.numpy()).all()
    one = recognize_image(host[0], ctx=ctx, glue=ctx.GLUE_NORMALIZE)
    assert (one["digits"] == out["digits"][0].cpu().numpy()).all() and len(one["grid"]) == 9
    # run.py's own glue (preprocess_cell) end to end
    c0 = o.find_grid_contour(o.preprocess_for_grid_detection(host[0]))
    proc = o.preprocess_cells(o.warp_cells(host[0], c0.astype(np.float32)))
    ed = cnn_oracle.predict(sd, o.cells_to_input(proc)[:, None])[1].numpy()
    assert (recognize_image(host[0], ctx=ctx)["digits"] == ed).all()
    assert recognize_image(host[3], ctx=ctx) is None


def test_preprocess_cells_and_runpy_glue(ctx, golden_dir):
    """N1: run.py's preprocess_cell (CLAHE + adaptive threshold) on the GPU, bit-exact; and the CNN fed through it."""
    rs = np.random.RandomState(17)
    frames, corners, _ = _frames(2, 540, 960, seed=41)
    real = np.concatenate([o.warp_cells(f, c) for f, c in zip(frames.cpu().numpy(), corners)])
    cells = np.concatenate([real, rs.randint(0, 256, (30, 28, 28)).astype(np.uint8), np.full((2, 28, 28), 200, np.uint8),
                            rs.randint(90, 110, (7, 28, 28)).astype(np.uint8)])
    d = torch.from_numpy(cells).cuda()
    got = ctx.preprocess_cells(d).cpu().numpy()
    exp = o.preprocess_cells(cells)
    assert (got == exp).all()
    g2 = np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz"))
    sd = {k: torch.from_numpy(g2[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS}
    ctx.load_state_dict(sd)
    logits, digits, conf = ctx.cnn_forward(d, want_digits=True, glue=ctx.GLUE_RUNPY)
    el, ed, ec = cnn_oracle.predict(sd, o.cells_to_input(exp)[:, None])
    assert np.abs(logits.cpu().numpy() - el.numpy()).max() <= LOGIT_TOL
    assert (digits.cpu().numpy() == ed.numpy()).all()


def test_is_cell_empty_batched(ctx):
    """N3: Otsu + ink ratio per cell, fp64 recurrence in the reference's order -> identical thresholds and ratios."""
    from sudoku_vision_amd.cv.extract import is_cell_empty
    rs = np.random.RandomState(23)
    frames, corners, _ = _frames(1, 540, 960, seed=43)
    cells = np.concatenate([o.warp_cells(frames[0].cpu().numpy(), corners[0]), rs.randint(0, 256, (20, 28, 28)).astype(np.uint8),
                            np.full((1, 28, 28), 200, np.uint8)])
    ratio, otsu = ctx.cell_ink_ratio(torch.from_numpy(cells).cuda())
    exp = [o.cell_ink_ratio(c) for c in cells]
    assert (otsu.cpu().numpy() == np.array([e[1] for e in exp])).all()
    assert np.allclose(ratio.cpu().numpy(), np.array([e[0] for e in exp], np.float32), rtol=0, atol=1e-7)
    for i in (0, 5, 40, 81, 101):
        assert is_cell_empty(cells[i]) == o.is_cell_empty(cells[i])


def test_resize_and_preprocess_cell_for_model(ctx):
    from sudoku_vision_amd.cv.extract import preprocess_cell_for_model
    rs = np.random.RandomState(29)
    for shape in ((40, 40), (28, 28), (17, 23), (64, 50)):
        img = rs.randint(0, 256, shape).astype(np.uint8)
        got = ctx.resize_linear(torch.from_numpy(img).cuda(), (28, 28)).cpu().numpy()
        assert (got == o.resize_linear(img, (28, 28))).all(), shape
        x = preprocess_cell_for_model(img)
        assert x.shape == (1, 28, 28) and x.dtype == np.float32
        assert (x[0] == o.resize_linear(img, (28, 28)).astype(np.float32) / 255.0).all()
    up = ctx.resize_linear(torch.from_numpy(img).cuda(), (100, 90)).cpu().numpy()
    assert (up == o.resize_linear(img, (100, 90))).all()


def test_error_behaviour_on_gpu(ctx):
    """Status codes -> exceptions: no weights, unsupported parameters, bad shapes; and the context survives them."""
    import sudoku_vision_amd as sva
    from sudoku_vision_amd._native import NativeError
    fresh = sva.Context()
    with pytest.raises(NativeError, match="SV_ERR_NO_WEIGHTS"):
        fresh.cnn_forward(torch.zeros((2, 1, 28, 28), device="cuda"))
    g = torch.zeros((1, 32, 32), dtype=torch.uint8, device="cuda")
    with pytest.raises(NativeError, match="SV_ERR_UNSUPPORTED"):
        fresh.blur(g, 9)
    with pytest.raises(NativeError, match="SV_ERR_BAD_ARG"):
        fresh.blur(g, 4)
    with pytest.raises(NativeError, match="SV_ERR_BAD_ARG"):
        fresh.adaptive_threshold(g, 10, 2)
    with pytest.raises(NativeError, match="SV_ERR_UNSUPPORTED"):
        fresh.adaptive_threshold(g, 33, 2)
    ctx.load_state_dict(cnn_oracle.random_state_dict(1))
    with pytest.raises(NativeError, match="SV_ERR_BAD_ARG"):
        ctx.cnn_forward(torch.zeros((1, 28, 28), dtype=torch.uint8, device="cuda"), glue=7)
    assert (fresh.blur(g, 5) == 0).all()                       # still usable
    fresh.close()


def test_frame_batches_end_at_the_grid_limit(ctx):
    """Every frame-batch entry takes at most 65535 frames (the launch grid's z limit) and says so as a bad shape, sv_gray_u8 included;
    65535 one-pixel frames still run.  The buffers are full size, so nothing depends on the check for its bounds."""
    from sudoku_vision_amd._native import NativeError
    rs = np.random.RandomState(3)
    px = rs.randint(0, 256, (65536, 1, 1, 3)).astype(np.uint8)
    frames = torch.from_numpy(px).cuda()
    for call in (ctx.gray, ctx.preprocess):
        with pytest.raises(NativeError, match="SV_ERR_BAD_ARG.*bad shape"):
            call(frames)
    got = ctx.gray(frames[:65535]).cpu().numpy()
    want = np.stack([o.gray(px[i]) for i in range(0, 65535, 257)])
    assert (got[::257] == want).all()


def test_tiny_and_odd_images(ctx):
    """Smallest shapes the reference's functions accept: every border path at once."""
    rs = np.random.RandomState(31)
    for H, W in ((1, 1), (2, 3), (5, 5), (11, 7), (16, 16), (17, 20), (33, 260)):
        img = rs.randint(0, 256, (1, H, W, 3)).astype(np.uint8)
        got = ctx.preprocess(torch.from_numpy(img).cuda()).cpu().numpy()
        assert (got[0] == o.preprocess_for_grid_detection(img[0])).all(), (H, W)


def _despeckle_np(img):
    """numpy/scipy statement of sv_despeckle_u8: two passes over 64x64 tiles (grid origin (0,0), then (-32,-32)); in every tile the
    8-connected components of the tile's own pixels that touch none of the tile's outermost pixels are erased.  It does not model the
    kernel's iteration cap (a tile whose fill needs more than MAX_IT iterations is left untouched): for inputs that come near it use
    tests/despeckle_ref.py, which does (tests/test_gpu_despeckle_topology.py)."""
    from scipy import ndimage
    out = (img > 0).copy()
    H, W = out.shape
    for off in (0, 32):
        for y0 in range(-off, H, 64):
            for x0 in range(-off, W, 64):
                ya, yb, xa, xb = max(y0, 0), min(y0 + 64, H), max(x0, 0), min(x0 + 64, W)
                t = out[ya:yb, xa:xb]
                if not t.any():
                    continue
                lab, n = ndimage.label(t, structure=np.ones((3, 3)))
                ring = np.zeros_like(t)
                if ya == y0:
                    ring[0] = True
                if yb == y0 + 64:
                    ring[-1] = True
                if xa == x0:
                    ring[:, 0] = True
                if xb == x0 + 64:
                    ring[:, -1] = True
                keep = np.unique(lab[ring & t])
                t &= np.isin(lab, keep[keep > 0])
    return out


def test_despeckle_equals_tile_labelling(ctx):
    """sv_despeckle_u8 / sv_despeckle_bits against a per-tile connected-component labelling in scipy, pixel for pixel: a synthetic frame,
    blobs, thin diagonals and a grid rotated by 45 degrees (the slow direction of either fill orientation), a frame of vertical and one of
    horizontal hairlines.  Exercises the transposing flood fill (tiles whose components reach deep into the tile along columns)."""
    from scipy import ndimage
    rs = np.random.RandomState(11)
    H, W = 384, 512
    imgs = []
    frames, _, _ = _frames(1, H, W, seed=52)
    imgs.append(ctx.preprocess(frames)[0].cpu().numpy() > 0)
    g = ndimage.gaussian_filter(rs.uniform(size=(H, W)), 1.5)
    imgs.append(g > np.quantile(g, 0.55))
    yy, xx = np.mgrid[:H, :W]
    imgs.append(((yy + xx) % 23 == 0) | ((yy - xx) % 31 == 0))                          # 1-px diagonals, both directions
    imgs.append((((yy + xx) % 41 < 3) | ((yy - xx) % 41 < 3)) & (abs(yy - H // 2) + abs(xx - W // 2) < 150))   # 45-degree grid in a diamond
    imgs.append((xx % 7 == 3) & (yy % 50 > 2))                                           # vertical hairlines, broken every 50 rows
    imgs.append((yy % 7 == 3) & (xx % 50 > 2))                                           # horizontal hairlines
    imgs.append(rs.uniform(size=(H, W)) < 0.3)                                           # dense noise
    d = torch.from_numpy((np.stack(imgs) * 255).astype(np.uint8)).cuda()
    got = ctx.despeckle(d).cpu().numpy() > 0
    bits = torch.from_numpy(np.packbits(np.stack(imgs), axis=2, bitorder="little").view(np.int32)).cuda()
    got_bits = np.unpackbits(ctx.despeckle_bits(bits).cpu().numpy().view(np.uint8).reshape(len(imgs), H, -1), axis=2, bitorder="little").astype(bool)
    for k, img in enumerate(imgs):
        want = _despeckle_np(img)
        assert np.array_equal(got[k], want), k
        assert np.array_equal(got_bits[k], want), k
    assert (got[6] != imgs[6]).any() and (got[1] != imgs[1]).any() and (got[0] != imgs[0]).any()   # something was erased at all


@pytest.mark.parametrize("H,W", [(130, 8192), (100, 8160), (70, 64), (200, 96)])
def test_despeckle_bits_widths(ctx, H, W):
    """sv_despeckle_bits on widths either side of what one 64-row band holds in the LDS (k_despeckle_bits_band up to 8,160 px, the tile-per-wave
    kernel beyond), one tile wide, and a width with an odd number of words per row; against the per-tile labelling."""
    rs = np.random.RandomState(H + W)
    yy, xx = np.mgrid[:H, :W]
    img = (rs.uniform(size=(H, W)) < 0.12) | (xx % 97 == 5) | (yy % 45 == 7)
    bits = torch.from_numpy(np.packbits(img[None], axis=2, bitorder="little").view(np.int32)).cuda()
    got = np.unpackbits(ctx.despeckle_bits(bits).cpu().numpy().view(np.uint8).reshape(1, H, -1), axis=2, bitorder="little").astype(bool)[0]
    want = _despeckle_np(img)
    assert np.array_equal(got, want) and (want != img).any()


def test_despeckle_preserves_grid_search(ctx):
    """The despeckle accelerator erases only whole components that sit strictly inside a 64x64 tile, and the host
    corner search returns the same answer on the filtered image (synthetic frames + adversarial blob images)."""
    import sudoku_vision_amd as sva
    from scipy import ndimage
    frames, corners, _ = _frames(6, 1080, 1920, seed=51)
    frames[4] = 180                                                        # no grid at all
    binary = ctx.preprocess(frames)
    filt = ctx.despeckle(binary)
    b, f = binary.cpu().numpy(), filt.cpu().numpy()
    assert ((f == 0) | (f == b)).all()                                     # only erases
    for i in range(6):
        a, c = sva.host.find_grid_corners(b[i]), sva.host.find_grid_corners(f[i])
        assert (a is None) == (c is None) and (a is None or (a == c).all())
    # bit-packed output (what crosses PCIe in the pipeline) = the byte output, and the host search on it agrees
    bits = torch.empty((6, 1080, 1920 // 32), dtype=torch.int32, device="cuda")
    ctx.despeckle(binary, out=torch.empty_like(binary), packed=bits)
    unpacked = np.unpackbits(bits.cpu().numpy().view(np.uint8).reshape(6, 1080, -1), axis=2, bitorder="little") * 255
    assert (unpacked == f).all()
    cb, fb = sva.host.find_grid_corners_bits_batch(bits.cpu().numpy(), 1080, 1920, threads=3)
    for i in range(6):
        a = sva.host.find_grid_corners(b[i])
        assert fb[i] == (a is not None) and (a is None or (cb[i] == a).all())
    lab, n = ndimage.label(b[0] > 0, structure=np.ones((3, 3)))
    kept = np.unique(lab[f[0] > 0])
    gone = np.setdiff1d(np.unique(lab[(b[0] > 0) & (f[0] == 0)]), [0])
    assert len(np.intersect1d(kept, gone)) == 0                            # components are erased whole or not at all
    objs = ndimage.find_objects(lab)
    for cid in gone[:: max(1, len(gone) // 300)]:
        sl = objs[cid - 1]
        assert sl[0].stop - sl[0].start <= 62 and sl[1].stop - sl[1].start <= 62
    assert len(gone) > 0.7 * n                                             # most specks are gone
    # adversarial shapes: random blobs at several densities, a spiral, a ring with an island, in-place operation
    rs = np.random.RandomState(3)
    imgs = []
    for thr in (0.4, 0.5, 0.6):
        g = ndimage.gaussian_filter(rs.uniform(size=(300, 420)), 2.0)
        imgs.append(((g > np.quantile(g, thr)) * 255).astype(np.uint8))
    sp = np.zeros((300, 420), np.uint8)
    for k in range(1, 14):                                                 # square spiral inside one tile
        sp[70 + 2 * k:70 + 2 * k + 1, 70 + 2 * k:130 - 2 * k] = 255
        sp[70 + 2 * k:130 - 2 * k, 130 - 2 * k - 1:130 - 2 * k] = 255
    sp[150:290, 40:400] = 255
    sp[160:280, 50:390] = 0
    sp[200:210, 200:210] = 255                                             # island inside the ring's hole
    imgs.append(sp)
    d = torch.from_numpy(np.stack(imgs)).cuda()
    out = d.clone()
    ctx.despeckle(out, out=out)                                            # in place
    fo = out.cpu().numpy()
    for img, fi in zip(imgs, fo):
        assert ((fi == 0) | (fi == img)).all()
        for mar in (0.1, 0.02):
            a, c = sva.host.find_grid_corners(img, mar), sva.host.find_grid_corners(fi, mar)
            assert (a is None) == (c is None) and (a is None or (a == c).all())


def test_bf16_configuration_digit_parity(golden_dir):
    """BASELINE configs[4]: bf16 MFMA conv2/fc1.  Parity target = digit indices; logits are compared loosely with the f32 model, and tightly
    with the emulation of the configuration's own rounding points (cnn_oracle.forward_bf16_emulated, the bound of test_gpu_cnn_accuracy.py)."""
    import sudoku_vision_amd as sva
    g2 = np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz"))
    sd = {k: torch.from_numpy(g2[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS}
    c = sva.Context()
    c.load_state_dict(sd)
    c.set_precision(c.PREC_BF16)
    frames, corners, _ = _frames(3, 540, 960, seed=61)
    cells = np.concatenate([o.warp_cells(f, cc) for f, cc in zip(frames.cpu().numpy(), corners)] +
                           [np.random.RandomState(5).randint(0, 256, (77, 28, 28)).astype(np.uint8)])
    for glue, x in ((0, o.cells_to_input(cells)), (1, o.cells_to_input(o.preprocess_cells(cells)))):
        logits, digits, conf = c.cnn_forward(torch.from_numpy(cells).cuda(), want_digits=True, glue=glue)
        el, ed, ec = cnn_oracle.predict(sd, x[:, None])
        err = np.abs(logits.cpu().numpy() - el.numpy())
        assert err.max() < 0.5 and err.mean() < 0.03, (err.max(), err.mean())
        top2 = np.sort(el.numpy(), 1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) > 4 * err.max()
        assert clear.mean() > 0.7
        assert (digits.cpu().numpy()[clear] == ed.numpy()[clear]).all()
        emu = cnn_oracle.forward_bf16_emulated(sd, cells, glue).numpy()
        noise = np.abs(cnn_oracle.forward_bf16_emulated(sd, cells, glue, acc=torch.float32).numpy() - emu).max()
        emu_err = np.abs(logits.cpu().numpy() - emu).max()
        slack = cnn_oracle.BF16_RUNPY_SLACK * np.abs(emu).max() if glue == 1 else 0.0
        assert emu_err <= cnn_oracle.tolerance(emu, noise, cnn_oracle.C_BF16) + slack, (glue, emu_err, noise)
    # the two fc kernels of this configuration against each other: a cell's logits do not depend on the batch it sits in, and both kernels add the
    # 98 K steps in the same order -- 97 cells per CU runs k_fc_head_bf16, its first 256 frames' worth alone runs k_fc_head_bf16p; 96 * 256 + 1
    # cells run k_fc_head_bf16 again, with a last tile of one cell (its clamp of the rows past the end of the batch)
    big = np.random.RandomState(6).randint(0, 256, (97 * 256, 28, 28)).astype(np.uint8)
    big[::3] = np.clip(big[::3].astype(int) // 4 + 150, 0, 255).astype(np.uint8)
    d = torch.from_numpy(big).cuda()
    l_all, dg_all, _ = c.cnn_forward(d, want_digits=True)
    for n in (96 * 256 + 1, 81 * 256, 81 * 256 - 19, 3000, 81):
        l_n, dg_n, _ = c.cnn_forward(d[:n], want_digits=True)
        assert torch.equal(l_n, l_all[:n]) and torch.equal(dg_n, dg_all[:n]), n
        assert (digits.cpu().numpy() == ed.numpy()).mean() > 0.97
    with pytest.raises(sva._native.NativeError, match="SV_ERR_UNSUPPORTED"):
        c.cnn_forward(torch.zeros((2, 1, 28, 28), device="cuda"))
    c.set_precision(c.PREC_F32)                       # and back: exact path again
    logits = c.cnn_forward(torch.from_numpy(cells).cuda())
    assert np.abs(logits.cpu().numpy() - cnn_oracle.forward(sd, o.cells_to_input(cells)[:, None]).numpy()).max() <= LOGIT_TOL
    c.close()


def test_stages_are_deterministic(ctx):
    """K1 (bytes and bits), the speck filter, the sparse records and K2 give the same bits twice on 64 1080p frames: a launch that fills every
    CU several times over (what test_cnn_is_deterministic does for K3)."""
    import sudoku_vision_amd as sva
    from sudoku_vision_amd import host
    frames, corners, _ = _frames(64, 1080, 1920, seed=77)
    minv = ctx.minv_to_device(sva.Context.corners_to_minv(corners))
    rec_bytes = host.sparse_bits_record_bytes(1080, 1920, 1080 * 60 // 3)

    def once():
        b = ctx.preprocess(frames)
        bits = ctx.preprocess_bits(frames)
        filt = ctx.despeckle_bits(bits.clone())
        rec = ctx.pack_sparse_bits(filt, torch.zeros((64, rec_bytes), dtype=torch.uint8, device="cuda")).clone()
        cells = ctx.warp_cells(frames, minv)
        return b, bits, filt, rec, cells

    first = once()
    for _ in range(3):
        for a, b in zip(first, once()):
            assert torch.equal(a, b)


def test_cnn_is_deterministic():
    """The same batch twice gives the same bits, for every kernel family of the product, at batch sizes where two workgroups share a CU (600 and
    2,000 cells for the two-cells-per-workgroup bf16 conv kernel) -- round 3 found the bf16 configuration's logits varying from run to run in the
    last bits of 6 % of the cells (k3_cnn_bf16.hip, note at conv1)."""
    import sudoku_vision_amd as sva
    from sudoku_vision_amd.synth import random_state_dict
    cells = torch.from_numpy(np.random.RandomState(6).randint(0, 256, (2000, 28, 28)).astype(np.uint8)).cuda()
    for setup in ("default", "bf16", "f32mfma"):
        c = sva.Context()
        c.load_state_dict(random_state_dict(3))
        if setup == "bf16":
            c.set_precision(c.PREC_BF16)
        elif setup == "f32mfma":
            c.set_cnn_kernels(c.CNN_F32MFMA)
        for n in (2000, 600):
            a = c.cnn_forward(cells[:n]).clone()
            for _ in range(5):
                assert torch.equal(c.cnn_forward(cells[:n]), a), (setup, n)


def _xctx():
    """A context of the test-only superset library (cross-check kernels, include/sudoku_vision_xcheck.h)."""
    import sudoku_vision_amd as sva
    return sva.Context(library=sva._native.lib_xcheck())


def test_conv_algorithms_agree(ctx, golden_dir):
    """Four independent conv2 (+ three fc1) implementations -- the product's f16 hi/lo operand pairs on the f16 matrix pipe
    (k3_cnn_h2.hip) and its f32-MFMA direct implicit GEMM (the kernels out-of-range inputs take), and the test-only library's Winograd
    stream on f32 MFMA and on bf16 MFMA with three-way operand splitting -- give the same logits to ~1e-5 and the same digits, and each is
    within 1e-4 of the PyTorch-CPU restatement (the default within 1e-5: its operand pairs carry 22 bits, its sums are f32).  The
    selection is a context setter (sv_ctx_set_cnn_kernels); nothing is read from the environment."""
    g = np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz"))
    sd = {k: torch.from_numpy(g[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS}
    cells = np.random.RandomState(1).randint(0, 256, (81 * 64 + 500, 28, 28)).astype(np.uint8)
    want = cnn_oracle.forward(sd, o.cells_to_input(cells)[:, None]).numpy()
    x = torch.from_numpy(cells).cuda()
    outs = []
    ctx.load_state_dict(sd)
    for which, name in ((ctx.CNN_AUTO, "auto"), (ctx.CNN_F16PAIR, "f16 pairs"), (ctx.CNN_F32MFMA, "f32 mfma")):
        ctx.set_cnn_kernels(which)
        assert ctx.conv_kernel_info()["algo"] == (0 if which == ctx.CNN_F32MFMA else 4)
        outs.append(ctx.cnn_forward(x).cpu().numpy())
        assert np.abs(outs[-1] - want).max() <= (LOGIT_TOL if which == ctx.CNN_F32MFMA else 1e-5), name
    ctx.set_cnn_kernels(ctx.CNN_AUTO)
    assert np.array_equal(outs[0], outs[1])                          # trained weights are in range: auto = the f16-pair kernels
    xc = _xctx()
    xc.load_state_dict(sd)
    for which, frame_fc in ((xc.CNN_X_WINOGRAD, 0), (xc.CNN_X_WSPLIT, 0), (xc.CNN_F32MFMA, 1), (xc.CNN_X_WINOGRAD, 1)):
        xc.set_cnn_kernels(which)
        xc._check(xc._lib.svx_ctx_set_fc_frame_kernel(xc._h, frame_fc), "svx_ctx_set_fc_frame_kernel")
        outs.append(xc.cnn_forward(x).cpu().numpy())
        assert np.abs(outs[-1] - want).max() <= LOGIT_TOL, (which, frame_fc)
    xc.close()
    for other in outs[1:]:
        assert np.abs(outs[0] - other).max() <= 2e-5
        assert (outs[0].argmax(1) == other.argmax(1)).all()


def test_cnn_has_the_reference_domain(ctx):
    """ml/model.py:34-42 accepts any f32 tensor and any weights.  The f16-pair kernels carry inputs and activations as f16 pairs
    (|v| < 65,504): with weights that push conv1's activations past that, and with f32 inputs far outside [-1, 1] or tiny, SV_CNN_AUTO
    must still deliver the oracle's logits (relative 1e-4 of the logits' scale) -- by switching to the f32-MFMA kernels, at load time
    for the weights and on the device per call for the inputs -- where the f16-pair kernels forced on the same data overflow."""
    import sudoku_vision_amd as sva
    rs = np.random.RandomState(5)
    sd = {k: v.clone() for k, v in cnn_oracle.random_state_dict(77).items()}
    c = sva.Context()

    def rel_err(got, want):
        return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))

    cells = rs.randint(0, 256, (300, 28, 28)).astype(np.uint8)
    x8 = o.cells_to_input(cells)[:, None]
    # (1) weights: conv1 scaled so that its activations reach ~1e6
    big = {k: v.clone() for k, v in sd.items()}
    big["conv1.weight"] *= 3.0e6
    c.load_state_dict(big)
    assert c.conv_kernel_info()["algo"] == 0                         # decided when the weights were loaded
    want = cnn_oracle.forward(big, x8).numpy()
    assert np.isfinite(want).all() and np.abs(want).max() > 1e4
    got = c.cnn_forward(torch.from_numpy(cells).cuda()).cpu().numpy()
    assert np.isfinite(got).all() and rel_err(got, want) <= 1e-4
    c.set_cnn_kernels(c.CNN_F16PAIR)                                 # the same through the f16-pair kernels: out of their range
    bad = c.cnn_forward(torch.from_numpy(cells).cuda()).cpu().numpy()
    assert not np.isfinite(bad).all() or rel_err(bad, want) > 1e-2
    c.set_cnn_kernels(c.CNN_AUTO)
    # (2) inputs: ordinary weights, f32 inputs of magnitude ~1e5, ~1e-6, with an Inf, and in range
    c.load_state_dict(sd)
    assert c.conv_kernel_info()["algo"] == 4
    base = rs.uniform(-1, 1, (200, 1, 28, 28)).astype(np.float32)
    for scale, tol in ((1.0e5, 1e-4), (1.0e-6, 1e-4), (1.0, 1e-5)):
        x = torch.from_numpy(base * np.float32(scale))
        want = cnn_oracle.forward(sd, x).numpy()
        got = c.cnn_forward(x.cuda()).cpu().numpy()
        assert np.isfinite(got).all() and rel_err(got, want) <= tol, scale
    x = torch.from_numpy(base.copy())
    x[3, 0, 5, 5] = float("inf")
    want = cnn_oracle.forward(sd, x).numpy()
    got = c.cnn_forward(x.cuda()).cpu().numpy()
    ok = np.isfinite(want).all(1)
    assert not ok[3] and ok.sum() == 199                             # the reference propagates the Inf into that cell's logits only
    # (that cell's own logits are unspecified here: ReLU / max-pool are v_max, which drops a NaN where torch keeps it); every other cell
    # of the batch is computed as if the Inf were not there
    assert rel_err(got[ok], want[ok]) <= 1e-4
    c.close()


def test_cnn_large_batch_frame_kernel(ctx, golden_dir):
    """A batch of more than 64 frames' cells with a ragged tail (the round-1 frame-per-workgroup fc kernel switched in here; it now lives in
    the test-only library, see test_conv_algorithms_agree)."""
    g2 = np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz"))
    sd = {k: torch.from_numpy(g2[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS}
    B = 81 * 64 + 37
    cells = np.random.RandomState(37).randint(0, 256, (B, 28, 28)).astype(np.uint8)
    cells[::3] = np.clip(cells[::3].astype(int) // 4 + 150, 0, 255).astype(np.uint8)
    _check_cnn(ctx, sd, cells)


@pytest.mark.parametrize("B", [81 * 256, 81 * 256 + 37, 41 * 256 + 5, 96 * 256, 96 * 256 + 1, 128 * 256])
def test_cnn_batches_of_the_per_cu_fc_kernel(ctx, golden_dir, B):
    """The fc head runs as k_fc_head_h2p (one workgroup per CU, the weight image streamed once, operands by LDS-DMA) while a CU's share of the
    cells fits one 96-cell pass, as k_fc_head_h2 beyond: the bench's batch (256 frames: 81 cells per CU, a sixth M tile with one row), a ragged
    one, a mid-size one (three M tiles per workgroup), the largest one-pass batch, the first past it and 512 frames; every cell against the
    oracle, trained weights (digit indices exact) and random weights.  (The small batches of the other CNN tests run k_fc_head_h2p too.)"""
    g2 = np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz"))
    sd = {k: torch.from_numpy(g2[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS}
    rs = np.random.RandomState(B % 1000)
    cells = rs.randint(0, 256, (B, 28, 28)).astype(np.uint8)
    cells[::3] = np.clip(cells[::3].astype(int) // 4 + 150, 0, 255).astype(np.uint8)
    _check_cnn(ctx, sd, cells)
    if B == 81 * 256 + 37:
        _check_cnn(ctx, cnn_oracle.random_state_dict(77), cells)


@pytest.mark.parametrize("H,W", [(3648, 2736), (123, 1000), (64, 244)])
def test_preprocess_other_resolutions(ctx, H, W):
    """The reference's test photos are 2736x3648 portrait; plus widths whose last 240-column strip is partial."""
    rs = np.random.RandomState(H + W)
    base = rs.randint(0, 256, (H // 8 + 2, W // 8 + 2, 3)).astype(np.uint8)
    img = np.repeat(np.repeat(base, 8, 0), 8, 1)[:H, :W].copy()          # blocky structure + noise: edges everywhere
    img = np.clip(img.astype(np.int16) + rs.randint(-12, 13, img.shape), 0, 255).astype(np.uint8)
    got = ctx.preprocess(torch.from_numpy(img[None]).cuda()).cpu().numpy()[0]
    assert (got == o.preprocess_for_grid_detection(img)).all()


def test_real_photo_end_to_end(ctx, golden_dir):
    """data/test_images/sample_4.jpg (the photo the reference's tests/test_integration.py:121 uses; committed as a data
    fixture, decoded with PIL on both sides): K1 at 2736x3648, host corner search, K2, run.py glue, CNN with the trained
    weights -- binary and cells bit-exact, digit indices equal to the oracle's."""
    from PIL import Image
    import sudoku_vision_amd as sva
    from sudoku_vision_amd.pipeline import recognize_image
    img = np.asarray(Image.open(os.path.join(golden_dir, "sample_4.jpg")).convert("RGB"))[..., ::-1].copy()
    assert img.shape == (3648, 2736, 3)
    g2 = np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz"))
    sd = {k: torch.from_numpy(g2[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS}
    ctx.load_state_dict(sd)
    d = torch.from_numpy(img).cuda()[None]
    binary = ctx.preprocess(d)[0].cpu().numpy()
    assert (binary == o.preprocess_for_grid_detection(img)).all()
    corners = sva.host.find_grid_corners(binary)
    assert corners is not None and (corners == o.find_grid_contour(binary)).all()
    minv = ctx.minv_to_device(sva.Context.corners_to_minv(corners[None].astype(np.float32)))
    cells = ctx.warp_cells(d, minv)[0].cpu().numpy()
    assert (cells == o.warp_cells(img, corners.astype(np.float32))).all()
    res = recognize_image(img, ctx=ctx, top_k=3)                          # run.py order incl. preprocess_cell
    el, ed, ec = cnn_oracle.predict(sd, o.cells_to_input(o.preprocess_cells(cells))[:, None])
    assert (res["digits"] == ed.numpy()).all()
    assert np.abs(res["logits"] - el.numpy()).max() <= LOGIT_TOL
    tp, ti = torch.softmax(el, 1).topk(3)                                 # run_v2's alternatives (run_v2.py:165-178)
    for i in range(81):
        assert [a for a, _ in res["alternatives"][i]] == ti[i, 1:].tolist()
        assert np.allclose([p for _, p in res["alternatives"][i]], tp[i, 1:].numpy(), atol=1e-5)


@pytest.mark.parametrize("k", [1, 3, 10])
def test_softmax_topk_matches_torch(ctx, k):
    """run_v2's epilogue (pipeline/run_v2.py:165-178): F.softmax + topk; indices exact, probabilities <= 1e-6 (f32).
    Checker = torch on the CPU, the library the reference itself calls."""
    rs = np.random.RandomState(k)
    logits = (rs.randn(81 * 7 + 5, 10) * 6).astype(np.float32)
    logits[3] = np.arange(10, dtype=np.float32)                       # ordered
    logits[4] = -np.arange(10, dtype=np.float32) * 9                  # near-saturated softmax, still no exact ties
    idx, prob = ctx.softmax_topk(torch.from_numpy(logits).cuda(), k)
    want_p, want_i = torch.softmax(torch.from_numpy(logits), 1).topk(k)
    assert (idx.cpu().numpy() == want_i.numpy()).all()
    assert np.abs(prob.cpu().numpy() - want_p.numpy()).max() <= 1e-6


def test_softmax_topk_bad_k(ctx):
    with pytest.raises(RuntimeError):
        ctx.softmax_topk(torch.zeros((4, 10), device="cuda"), 11)


def test_full_size_batch_properties(ctx, golden_dir):
    """BASELINE configs[1] at full size (256 synthetic 1080p frames, the bench's seed): size-independent properties of the
    whole path, plus an oracle spot check on three frames of the batch.
      * K1 output is binary and identical whether a frame is processed alone, in a ragged sub-batch or in the full batch;
      * K2 cells likewise (bit-exact); digits equal, logits within 1e-5 across batch shapes (the fc kernel's summation order
        depends on the batch size, the conv kernel's does not);
      * round-robin shards (N = 2, 3, 8) recombine to the unsharded result -- the multi-GPU partitioning loses nothing;
      * frames 0, 101 and 255 against the oracle: binary and cells bit-exact, logits <= 1e-4, digits equal."""
    import sudoku_vision_amd as sva
    from sudoku_vision_amd import sharding
    g2 = np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz"))
    sd = {k: torch.from_numpy(g2[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS}
    ctx.load_state_dict(sd)
    n = 256
    frames, corners, _ = _frames(n, 1080, 1920, seed=1234)
    minv = ctx.minv_to_device(sva.Context.corners_to_minv(corners))
    binary = ctx.preprocess(frames)
    vals = torch.unique(binary)
    assert set(vals.cpu().tolist()) <= {0, 255}
    full = ctx.frames_to_digits(frames, minv, keep_cells=True)
    full = {k: v.clone() for k, v in full.items()}
    # ragged sub-batches and a lone frame
    for lo, hi in ((0, 100), (100, 256), (17, 18)):
        assert torch.equal(ctx.preprocess(frames[lo:hi]), binary[lo:hi])
        part = ctx.frames_to_digits(frames[lo:hi], minv[lo:hi], keep_cells=True)
        assert torch.equal(part["cells"], full["cells"][lo:hi])
        assert torch.equal(part["digits"], full["digits"][lo:hi])
        assert (part["logits"] - full["logits"][lo:hi]).abs().max().item() <= 1e-5
    # round-robin shards recombine
    for world in (2, 3, 8):
        digits = torch.empty_like(full["digits"])
        for rank in range(world):
            idx = torch.tensor(sharding.shard_indices(n, rank, world), device="cuda")
            part = ctx.frames_to_digits(frames[idx].contiguous(), minv[idx].contiguous())
            digits[idx] = part["digits"]
        assert torch.equal(digits, full["digits"])
    # oracle spot check
    for i in (0, 101, 255):
        host = frames[i].cpu().numpy()
        assert (binary[i].cpu().numpy() == o.preprocess_for_grid_detection(host)).all()
        cells = o.warp_cells(host, corners[i])
        assert (full["cells"][i].cpu().numpy() == cells).all()
        el, ed, ec = cnn_oracle.predict(sd, o.cells_to_input(cells)[:, None])
        assert np.abs(full["logits"][i].cpu().numpy() - el.numpy()).max() <= LOGIT_TOL
        assert (full["digits"][i].cpu().numpy() == ed.numpy()).all()


@pytest.mark.parametrize("row_pad,frame_gap", [(64, 0), (20, 0), (7, 0), (64, 4096), (12, 100)])
def test_padded_rows_and_frame_gaps(ctx, golden_dir, row_pad, frame_gap):
    """Camera buffers are rarely dense: the C ABI takes a row pitch and a frame stride.  Frames embedded in a larger buffer with
    `row_pad` bytes after every row and `frame_gap` bytes between frames (garbage in the padding) give the same binary, cells and
    digits as the dense copy -- through the 4-byte-aligned marching K1 (pad 64), the tiled fallback (pads 20, 12) and the
    unaligned-pitch path (pad 7)."""
    import sudoku_vision_amd as sva
    g2 = np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz"))
    ctx.load_state_dict({k: torch.from_numpy(g2[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS})
    n, H, W = 3, 270, 480
    dense, corners, _ = _frames(n, H, W, seed=row_pad + frame_gap)
    pitch = 3 * W + row_pad
    fstride = pitch * H + frame_gap
    buf = torch.randint(0, 256, (n * fstride + 64,), dtype=torch.uint8, device="cuda")       # garbage everywhere first
    view = torch.as_strided(buf, (n, H, W, 3), (fstride, pitch, 3, 1))
    view.copy_(dense)
    assert not view.is_contiguous()
    minv = ctx.minv_to_device(sva.Context.corners_to_minv(corners))
    assert torch.equal(ctx.preprocess(view), ctx.preprocess(dense))
    assert torch.equal(ctx.gray(view), ctx.gray(dense))
    assert torch.equal(ctx.warp_cells(view, minv), ctx.warp_cells(dense, minv))
    a, b = ctx.frames_to_digits(view, minv), ctx.frames_to_digits(dense, minv)
    assert torch.equal(a["digits"], b["digits"]) and torch.equal(a["logits"], b["logits"])
    assert (ctx.preprocess(dense)[0].cpu().numpy() == o.preprocess_for_grid_detection(dense[0].cpu().numpy())).all()


@pytest.mark.parametrize("H,W,kind", [(1080, 1920, "synthetic"), (1080, 1920, "noise"), (540, 960, "synthetic"), (64, 128, "noise"), (33, 48, "noise"),
                                      (100, 272, "noise"), (16, 16, "noise"), (200, 144, "flat")])
def test_k1_matrix_pipe_form(ctx, H, W, kind):
    """K1 in its second, independent formulation (csrc/k1_threshold_mm.hip: Toeplitz GEMMs on the f16 MFMA, approximate local mean, exact
    re-decision of the pixels the approximation cannot decide) against the oracle, bit for bit; and the approximation error the scheme's
    EPS = 2^-9 rests on, measured against a float64 evaluation of the same Gaussian on the oracle's blurred image."""
    from scipy import ndimage
    if kind == "synthetic":
        frames = _frames(2, H, W, seed=H + W)[0]
    elif kind == "noise":
        frames = torch.randint(0, 256, (2, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(H * W)).to(ctx.device)
        frames[1] = (frames[1].float() * 0.1 + 100).to(torch.uint8)               # low-contrast noise: many means close to src + 1.5
    else:
        frames = torch.full((2, H, W, 3), 90, dtype=torch.uint8, device=ctx.device)
        frames[1, :, : W // 2] = 97
    xc = _xctx()                                                                  # the matrix-pipe K1 lives in the test-only library
    xc.preprocess_stats()                                                         # switches the counter on / resets it
    binary, mean = xc.preprocess_mm(frames, want_mean=True)
    redecided, _ = xc.preprocess_stats()
    host = frames.cpu().numpy()
    taps = o.gaussian_kernel_f32(11).astype(np.float64)
    worst = 0.0
    for i in range(2):
        assert (binary[i].cpu().numpy() == o.preprocess_for_grid_detection(host[i])).all(), (H, W, kind, i)
        blurred = o.gaussian_blur(o.gray(host[i]), 5).astype(np.float64)
        ref = ndimage.correlate1d(ndimage.correlate1d(blurred, taps, axis=1, mode="nearest"), taps, axis=0, mode="nearest")
        worst = max(worst, float(np.abs(mean[i].cpu().numpy().astype(np.float64) - ref).max()))
    assert worst < 4e-4, worst                   # the float64 sum is itself within 1.5e-4 of cv2's float chain; EPS is 1.95e-3
    assert torch.equal(binary, ctx.preprocess(frames))
    assert redecided < 0.02 * 2 * H * W + 64, redecided


@pytest.mark.parametrize("H,W", [(2160, 3840), (720, 1280)])
def test_pipeline_other_resolutions(ctx, H, W):
    """FramePipeline end to end on 4K (two mask groups per row in the sparse records, 4320 row groups: the pack kernel's streaming form) and
    720p frames: every grid found, corners equal to the plain search on K1's binary, digits equal to the device-only path."""
    import sudoku_vision_amd as sva
    from sudoku_vision_amd import synth
    from sudoku_vision_amd.pipeline import FramePipeline
    ctx.load_state_dict(synth.random_state_dict(1234))
    frames, corners, _ = synth.synth_frames(5, H, W, seed=H, device=ctx.device)
    pipe = FramePipeline(ctx, H, W, chunk=2, host_threads=3)
    assert pipe.packed
    out = pipe.run(frames)
    torch.cuda.synchronize()
    binary = ctx.preprocess(frames).cpu().numpy()
    for i in range(5):
        want = sva.host.find_grid_corners(binary[i])
        assert want is not None and out["found"][i] and (out["corners"][i] == want).all()
    minv = ctx.minv_to_device(sva.Context.corners_to_minv(out["corners"].astype(np.float32)))
    assert torch.equal(out["digits"], ctx.frames_to_digits(frames, minv)["digits"])
