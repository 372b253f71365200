"""GPU (-m gpu): reduced-size JPEG decode (reduce = 2, 4, 8; csrc/k5_jpeg.hip: k_jpeg_idct4, k_jpeg_idct_small<2>, <1>, k_jpeg_idct on
4:2:0 chroma at reduce = 2, and k_jpeg_colour, the colour kernel of every scale) against Pillow's libjpeg-turbo decode at the same scale
(tests/test_jpeg_reduced_ref.py::pil_reduced_bgr, which asserts that Pillow did reduce by d).  Exact equality, through the compact and
the dense transport.  tests/test_jpeg_reduced_ref.py checks the same files against the numpy restatement on the CPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cnn_oracle
import sv_oracle as o
import test_jpeg_crafted as T
from test_jpeg_reduced_ref import DENOMS, SCALES, crafted_files, orientation_cases, pil_reduced_bgr, synth_file

pytestmark = pytest.mark.gpu

SAMPLINGS = ("gray", 0, 1, 2)                                                 # gray, 4:4:4, 4:2:2, 4:2:0


def assert_equals_pillow(ctx, data, d, what=""):
    want = pil_reduced_bgr(data, d)
    for dense in (False, True):
        got = ctx.imdecode(data, dense=dense, reduce=d).cpu().numpy()
        assert got.shape == want.shape, (what, d, dense, got.shape, want.shape)
        assert (got == want).all(), (what, d, dense, int((got != want).sum()))
    return want


@pytest.mark.parametrize("d", DENOMS)
@pytest.mark.parametrize("sub", SAMPLINGS)
def test_reduced_synthetic(ctx, sub, d):
    """(61, 83): partial MCUs, odd reduced sizes; (17, 9): reduced 4:2:2 chroma at most 2 wide (replication), one-block-wide components;
    (64, 80): whole MCUs"""
    for h, w in ((61, 83), (17, 9), (64, 80)):
        assert_equals_pillow(ctx, synth_file(h, w, sub), d, (h, w))


@pytest.mark.parametrize("d", DENOMS)
def test_reduced_crafted(ctx, d):
    """hard chroma at the sizes where the up-sampling filter changes form, rank selection (restart intervals too), block counts at
    component and workgroup boundaries, every (Cb, Cr) pair"""
    for name, data in crafted_files():
        assert_equals_pillow(ctx, data, d, name)


@pytest.mark.parametrize("d", DENOMS)
def test_reduced_range_limit(ctx, d):
    """T.file_d, judged as tests/test_jpeg_reduced_ref.py::test_restatement_range_limit judges the restatement: by Pillow up to k = 511"""
    f = T.file_d()
    ks = np.array(T.d_offsets())
    S = 8 // d
    keep = np.repeat(ks <= 511, S)
    want = pil_reduced_bgr(f.data, d)
    for dense in (False, True):
        got = ctx.imdecode(f.data, dense=dense, reduce=d).cpu().numpy()
        assert got.shape == want.shape == (S, S * len(ks), 3)
        assert (got[:, keep] == want[:, keep]).all(), dense


@pytest.mark.parametrize("orient", [1, 3, 6, 8])
def test_reduced_orientations(ctx, orient):
    data = synth_file(61, 83, 2, orient)
    want = assert_equals_pillow(ctx, data, 2, orient)
    assert want.shape == ((42, 31, 3) if orient >= 5 else (31, 42, 3))


@pytest.mark.parametrize("d", SCALES)
def test_orientations_samplings_scales(ctx, d):
    """every EXIF orientation x gray, 4:4:4, 4:2:2, 4:2:0 at scale 1 / d, both transports: the cases
    tests/test_jpeg_reduced_ref.py::test_restatement_orientations_samplings_scales holds the restatement to on the CPU"""
    for what, data, want in orientation_cases(d):
        for dense in (False, True):
            got = ctx.imdecode(data, dense=dense, reduce=d).cpu().numpy()
            assert got.shape == want.shape, (what, dense, got.shape, want.shape)
            assert (got == want).all(), (what, dense, int((got != want).sum()))


def test_scaled_entries_at_one_are_the_unscaled_entries(ctx):
    """the C entry points called directly: sv_jpeg_reconstruct[_sparse]_scaled_bgr_u8 at scale_denom = 1 write the bytes
    sv_jpeg_reconstruct[_sparse]_bgr_u8 write (the oracle's) into a buffer with padded rows, and nothing outside the rows"""
    from sudoku_vision_amd import _native, host
    lib = _native.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream)
    for sub in (2, "gray"):
        data = synth_file(61, 83, sub)
        want = o.imdecode(data)
        H, W = want.shape[:2]
        assert (H, W) == (61, 83)
        info, coef, quant = host.jpeg_entropy_decode(data)
        _, masks, offs, vals, _ = host.jpeg_entropy_decode_sparse(data)
        dquant, dcoef = torch.from_numpy(quant.view(np.int16)).to(ctx.device), torch.from_numpy(coef).to(ctx.device)
        dm, do, dv = (torch.from_numpy(a.view(t)).to(ctx.device) for a, t in ((masks, np.int64), (offs, np.int32), (vals, np.int16)))
        pitch, offset = 3 * W + 37, 1001
        inside = np.zeros(offset + H * pitch + 333, bool)
        inside[((offset + pitch * np.arange(H))[:, None] + np.arange(3 * W)).ravel()] = True
        for name, coefs in (("sv_jpeg_reconstruct%s_bgr_u8", (p(dcoef),)), ("sv_jpeg_reconstruct_sparse%s_bgr_u8", (p(dm), p(do), p(dv)))):
            hosts = []
            for scaled in (False, True):
                buf = torch.full((inside.size,), 0xA5, dtype=torch.uint8, device=ctx.device)
                args = (ctx._h, C.byref(info), *coefs, p(dquant), C.c_void_p(buf.data_ptr() + offset), pitch, stream)
                fn = getattr(lib, name % ("_scaled" if scaled else ""))
                _native.check(fn(*args, 1) if scaled else fn(*args), fn.__name__)
                hosts.append(buf.cpu().numpy())
                assert (hosts[-1][inside].reshape(H, W, 3) == want).all(), (sub, name, scaled)
                assert (hosts[-1][~inside] == 0xA5).all(), (sub, name, scaled)
            assert (hosts[0] == hosts[1]).all(), (sub, name)


def test_reduced_out_with_pitch(ctx):
    """imdecode(out=view, reduce=2) at orientation 6 into a strided view with padded rows: Pillow's pixels inside, nothing changed outside"""
    data = synth_file(61, 83, 2, 6)
    want = pil_reduced_bgr(data, 2)
    H, W = want.shape[:2]
    assert (H, W) == (42, 31)
    pitch, offset = 3 * W + 37, 1001
    for dense in (False, True):
        buf = torch.full((offset + H * pitch + 333,), 0xA5, dtype=torch.uint8, device=ctx.device)
        view = torch.as_strided(buf, (H, W, 3), (pitch, 3, 1), offset)
        ret = ctx.imdecode(data, out=view, dense=dense, reduce=2)
        assert ret.data_ptr() == view.data_ptr()
        host = buf.cpu().numpy()
        inside = np.zeros(host.shape, bool)
        inside[((offset + pitch * np.arange(H))[:, None] + np.arange(3 * W)).ravel()] = True
        assert (host[inside].reshape(H, W, 3) == want).all(), dense
        assert (host[~inside] == 0xA5).all(), dense
    with pytest.raises(ValueError, match="out must be"):
        ctx.imdecode(data, out=torch.empty((83, 61, 3), dtype=torch.uint8, device=ctx.device), reduce=2)


def test_reduced_batch(ctx):
    """imdecode_batch of mixed samplings and sizes at reduce = 4 against the single-image path (and Pillow); same shapes -> one tensor"""
    mixed = [synth_file(h, w, sub) for h, w, sub in ((50, 70, 0), (33, 97, 1), (128, 64, 2), (40, 56, "gray"))]
    for dense in (False, True):
        outs = ctx.imdecode_batch(mixed, threads=2, dense=dense, reduce=4)
        assert isinstance(outs, list)
        for data, t in zip(mixed, outs):
            single = ctx.imdecode(data, dense=dense, reduce=4)
            assert t.shape == single.shape and bool((t == single).all())
            assert (t.cpu().numpy() == pil_reduced_bgr(data, 4)).all()
    same = [synth_file(61, 83, sub) for sub in (2, 1, 0)]
    out = ctx.imdecode_batch(same, threads=3, reduce=4)
    assert tuple(out.shape) == (3, 16, 21, 3)
    for data, t in zip(same, out):
        assert (t.cpu().numpy() == pil_reduced_bgr(data, 4)).all()


def test_reduced_back_to_back(ctx):
    """different sizes and different d on one context, small before large: the component planes regrow between calls"""
    jobs = [(synth_file(64, 64, 2), 8), (synth_file(333, 222, 2), 2), (synth_file(90, 500, 1), 4), (synth_file(700, 900, 0), 2), (synth_file(200, 300, 2), 1)]
    outs = [ctx.imdecode(data, reduce=d) for data, d in jobs]
    for (data, d), t in zip(jobs, outs):
        want = pil_reduced_bgr(data, d) if d > 1 else o.imdecode(data)
        assert (t.cpu().numpy() == want).all(), d


def test_reduced_restart_intervals(ctx):
    for sub, kw in ((2, dict(restart_marker_blocks=3)), (0, dict(restart_marker_rows=1))):
        data = synth_file(96, 144, sub, **kw)
        assert o.jpeg_info(data).restart_interval > 0
        for d in DENOMS:
            assert_equals_pillow(ctx, data, d, sub)
            assert (ctx.imdecode(data, threads=2, reduce=d).cpu().numpy() == pil_reduced_bgr(data, d)).all()


def test_reduce_one_is_the_existing_decode(ctx):
    for h, w, sub in ((61, 83, 2), (17, 9, 1), (64, 80, 0), (40, 56, "gray")):
        data = synth_file(h, w, sub)
        for dense in (False, True):
            a, b = ctx.imdecode(data, dense=dense), ctx.imdecode(data, dense=dense, reduce=1)
            assert a.shape == b.shape and bool((a == b).all())
            assert (b.cpu().numpy() == o.imdecode(data)).all()


def test_imread_reduced_photo_then_recognise(ctx, golden_dir):
    """sample_1.jpg at reduce = 4 (the v1 corner search finds the grid in Pillow's 912 x 684 frame on the CPU oracle path, so 4 it is):
    equal to Pillow, and recognize_image returns a grid from the frame, on the host or left in HBM."""
    from sudoku_vision_amd import imgcodecs
    from sudoku_vision_amd.pipeline import recognize_image
    path = os.path.join(golden_dir, "sample_1.jpg")
    img = imgcodecs.imread(path, reduce=imgcodecs.reduce_from_flags(imgcodecs.IMREAD_REDUCED_COLOR_4))
    assert img.dtype == np.uint8 and img.shape == (912, 684, 3)
    assert (img == pil_reduced_bgr(open(path, "rb").read(), 4)).all()
    g2 = np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz"))
    ctx.load_state_dict({k: torch.from_numpy(g2[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS})
    a = recognize_image(img, ctx=ctx)
    b = recognize_image(imgcodecs.imread(path, device=True, reduce=4), ctx=ctx)
    assert a is not None and len(a["grid"]) == 9 and all(len(r) == 9 for r in a["grid"])
    assert (a["digits"] == b["digits"]).all() and (a["corners"] == b["corners"]).all()


def test_bad_reduce_is_a_value_error(ctx):
    from sudoku_vision_amd import imgcodecs
    data = synth_file(16, 16, 2)
    for bad in (3, 0, 16):
        with pytest.raises(ValueError, match="reduce"):
            ctx.imdecode(data, reduce=bad)
        with pytest.raises(ValueError, match="reduce"):
            ctx.imdecode_batch([data], reduce=bad)
        with pytest.raises(ValueError, match="reduce"):
            imgcodecs.imdecode(data, reduce=bad)
