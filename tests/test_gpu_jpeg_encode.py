"""GPU (-m gpu): the JPEG encoder (cv2.imwrite, pipeline/run.py:431).  The device half (csrc/k17_jpeg_encode.hip) against the restatement
tests/jpeg_encode_ref.py -- dense coefficients and the sparse records, exactly -- and the whole path (Context.imencode, imencode_batch,
imgcodecs.imencode / imwrite, recognize_stream(encode=True)) against Pillow's (libjpeg-turbo's) bytes."""
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_encode_ref as R

pytestmark = pytest.mark.gpu

COLOUR = ["444", "422", "420"]


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _pil_bgr(data):
    im = Image.open(io.BytesIO(data))
    return np.asarray(im) if im.mode == "L" else np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


@pytest.fixture(scope="module")
def references():
    """(sampling, kind, H, W, quality) -> (image, geometry, dense coefficients, sparse records): computed once, never changed"""
    cache = {}

    def get(sampling, kind, H, W, q):
        key = (sampling, kind, H, W, q)
        if key not in cache:
            img = R.content(kind, H, W, sampling == "gray")
            geo, coef, quant = R.forward(img, q, sampling)
            cache[key] = (img, geo, coef, R.sparse(coef))
        return cache[key]
    return get


@pytest.mark.parametrize("sampling", list(R.SAMPLINGS))
def test_device_half_equals_restatement(ctx, references, sampling):
    """dense coefficients bit for bit; masks, offsets, values and the per-frame count exactly.  Every size, quality and content of the case list
    (the restart interval does not reach the device half)."""
    for H, W in R.SIZES:
        for kind in R.CONTENTS:
            for q in R.QUALITIES:
                img, geo, coef, (masks, offsets, values) = references(sampling, kind, H, W, q)
                plan = ctx.jpeg_encode_plan(W, H, geo.ncomp, q, "444" if sampling == "gray" else sampling, 0)
                assert plan.info.coef_count == geo.coef_count
                frame = _dev(ctx, img)[None]
                dense = ctx.jpeg_forward(frame, plan, dense=True)
                assert (dense[0].cpu().numpy() == coef).all(), (H, W, kind, q)
                m, o, v, c = ctx.jpeg_forward(frame, plan)
                assert int(c[0]) == values.size, (H, W, kind, q)
                assert (m[0].cpu().numpy().view(np.uint64) == masks).all(), (H, W, kind, q)
                assert (o[0].cpu().numpy().view(np.uint32) == offsets).all(), (H, W, kind, q)
                assert (v[0, :values.size].cpu().numpy() == values).all(), (H, W, kind, q)


@pytest.mark.parametrize("sampling", list(R.SAMPLINGS))
def test_imencode_equals_pillow(ctx, sampling):
    s = "444" if sampling == "gray" else sampling
    for H, W in R.SIZES:
        for kind in R.CONTENTS:
            img = R.content(kind, H, W, sampling == "gray")
            frame = _dev(ctx, img)
            for q in R.QUALITIES:
                for restart in R.RESTARTS:
                    assert ctx.imencode(frame, q, s, restart) == R.pillow_encode(img, q, sampling, restart), (H, W, kind, q, restart)
    img = R.content("photo", 64, 64, sampling == "gray")
    assert ctx.imencode(_dev(ctx, img), 75, s) == R.pillow_encode(img, 75, sampling)
    assert ctx.imencode(_dev(ctx, img), 75, s, restart=2, threads=3) == R.pillow_encode(img, 75, sampling, 2)


def test_more_than_one_tile_and_scan_round(ctx):
    """300 x 700: six 128-pixel tiles a row, the last one partial; 9900 blocks at 4:4:4, three rounds of the prefix sum"""
    img = R.content("photo", 300, 700)
    for s in COLOUR:
        geo, coef, _ = R.forward(img, 90, s)
        masks, offsets, values = R.sparse(coef)
        plan = ctx.jpeg_encode_plan(700, 300, 3, 90, s, 0)
        m, o, v, c = ctx.jpeg_forward(_dev(ctx, img)[None], plan)
        assert int(c[0]) == values.size and (o[0].cpu().numpy().view(np.uint32) == offsets).all()
        assert (m[0].cpu().numpy().view(np.uint64) == masks).all() and (v[0, :values.size].cpu().numpy() == values).all()
        assert ctx.imencode(_dev(ctx, img), 90, s) == R.pillow_encode(img, 90, s), s
    gray = R.content("photo", 300, 700, gray=True)
    assert ctx.imencode(_dev(ctx, gray), 90) == R.pillow_encode(gray, 90, "gray")


def test_batch_equals_singles(ctx):
    H, W = 40, 56
    frames = [R.content(kind, H, W) for kind in ("noise", "checker", "zeros", "ramp", "photo")]
    batch = _dev(ctx, np.stack(frames))
    singles = [ctx.imencode(batch[i], 75, "420", 2) for i in range(5)]
    assert singles == [R.pillow_encode(f, 75, "420", 2) for f in frames]
    assert ctx.imencode_batch(batch, 75, "420", 2) == singles
    assert ctx.imencode_batch([batch[i] for i in range(5)], 75, "420", 2, threads=4) == singles
    old = ctx._ENC_CHUNK_BYTES
    try:
        ctx._ENC_CHUNK_BYTES = 1                                       # one frame per chunk
        assert ctx.imencode_batch(batch, 75, "420", 2, threads=2) == singles
    finally:
        ctx._ENC_CHUNK_BYTES = old
    with pytest.raises(ValueError):
        ctx.imencode_batch([batch[0], batch[1, :-8]])


def test_pitched_frames_and_views(ctx):
    """Views are accepted: rows of pitch 3 W + 13 are read in place, anything else is packed first; the bytes are those of the packed copy."""
    H, W = 33, 41
    img = R.content("noise", H, W)
    want = R.pillow_encode(img, 95, "420")
    buf = torch.zeros((H, 3 * W + 13), dtype=torch.uint8, device=ctx.device)
    buf[:, :3 * W] = _dev(ctx, img).view(H, 3 * W)
    pitched = buf[:, :3 * W].unflatten(1, (W, 3))
    assert pitched.stride() == (3 * W + 13, 3, 1) and not pitched.is_contiguous()
    assert ctx.imencode(pitched) == want
    wide = _dev(ctx, np.repeat(img, 2, axis=1))
    assert ctx.imencode(wide[:, ::2]) == want                          # every other pixel: not a dense row
    assert ctx.imencode(_dev(ctx, img[:, ::-1]).flip(1)) == want
    gbuf = torch.zeros((H, W + 7), dtype=torch.uint8, device=ctx.device)
    gbuf[:, :W] = _dev(ctx, img[..., 1])
    assert ctx.imencode(gbuf[:, :W], 75) == R.pillow_encode(img[..., 1], 75, "gray")
    with pytest.raises(TypeError):
        ctx.imencode(img)                                               # a numpy array is imgcodecs.imencode's business
    with pytest.raises(TypeError):
        ctx.imencode(_dev(ctx, img).float())
    for bad in ({"quality": 0}, {"quality": 101}, {"sampling": "411"}, {"restart": -1}, {"restart": 65536}):
        with pytest.raises(ValueError):
            ctx.imencode(_dev(ctx, img), **bad)


def test_1080p_equals_pillow(ctx):
    """1080 rows are 67.5 MCU rows at 4:2:0: the bottom luma block row of the last MCU row is made of dummy blocks"""
    img = R.content("photo", 1080, 1920)
    img = (img.astype(np.int32) + (np.arange(1920)[None, :, None] // 64 + np.arange(1080)[:, None, None] // 90) % 23).clip(0, 255).astype(np.uint8)
    assert ctx.imencode(_dev(ctx, img), 95, "420") == R.pillow_encode(img, 95, "420")


def test_round_trip_and_the_transport_form_is_the_decoders(ctx):
    from sudoku_vision_amd import _native
    for s in COLOUR:
        img = R.content("photo", 70, 100)
        data = ctx.imencode(_dev(ctx, img), 90, s)
        want = _pil_bgr(R.pillow_encode(img, 90, s))
        assert (ctx.imdecode(data).cpu().numpy() == want).all(), s
        # the encoder's records straight into the decoder's device half: no host in between
        plan = ctx.jpeg_encode_plan(100, 70, 3, 90, s, 0)
        m, o, v, c = ctx.jpeg_forward(_dev(ctx, img)[None], plan)
        quant = torch.from_numpy(np.array(plan.quant, np.uint16).view(np.int16).copy()).to(ctx.device)
        out = torch.zeros((70, 100, 3), dtype=torch.uint8, device=ctx.device)
        rc = ctx._lib.sv_jpeg_reconstruct_sparse_bgr_u8(ctx._h, C.byref(plan.info), m.data_ptr(), o.data_ptr(), v.data_ptr(), quant.data_ptr(), out.data_ptr(), 300,
                                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _native.check(rc, "sv_jpeg_reconstruct_sparse_bgr_u8", ctx._lib)
        assert (out.cpu().numpy() == want).all(), s


def test_imgcodecs_imencode_imwrite(ctx, tmp_path):
    from sudoku_vision_amd import imgcodecs as ic
    assert (ic.IMWRITE_JPEG_QUALITY, ic.IMWRITE_JPEG_PROGRESSIVE, ic.IMWRITE_JPEG_OPTIMIZE, ic.IMWRITE_JPEG_RST_INTERVAL, ic.IMWRITE_JPEG_SAMPLING_FACTOR) == (1, 2, 3, 4, 7)
    assert (ic.IMWRITE_JPEG_SAMPLING_FACTOR_420, ic.IMWRITE_JPEG_SAMPLING_FACTOR_422, ic.IMWRITE_JPEG_SAMPLING_FACTOR_444) == (0x221111, 0x211111, 0x111111)
    img = R.content("photo", 48, 80)
    path = str(tmp_path / "out.jpg")
    assert ic.imwrite(path, img, ctx=ctx) is True                      # numpy in; quality 95 and 4:2:0 when the caller says nothing
    assert open(path, "rb").read() == R.pillow_encode(img, 95, "420")
    with Image.open(path) as im:
        assert im.size == (80, 48) and im.mode == "RGB"
        im.load()
    assert ic.imwrite(path, _dev(ctx, img), [ic.IMWRITE_JPEG_QUALITY, 60, ic.IMWRITE_JPEG_SAMPLING_FACTOR, ic.IMWRITE_JPEG_SAMPLING_FACTOR_422,
                                              ic.IMWRITE_JPEG_RST_INTERVAL, 3, ic.IMWRITE_JPEG_OPTIMIZE, 0, ic.IMWRITE_JPEG_PROGRESSIVE, 0], ctx=ctx)
    assert open(path, "rb").read() == R.pillow_encode(img, 60, "422", 3)
    ok, buf = ic.imencode(".jpg", img[..., 0], [ic.IMWRITE_JPEG_QUALITY, 80], ctx=ctx)
    assert ok is True and buf.dtype == np.uint8 and buf.ndim == 1 and buf.tobytes() == R.pillow_encode(img[..., 0], 80, "gray")
    assert ic.imencode(".JPEG", img[..., :1], ctx=ctx)[1].tobytes() == R.pillow_encode(img[..., 0], 95, "gray")
    assert ic.imwrite(str(tmp_path / "no_such_dir" / "out.jpg"), img, ctx=ctx) is False
    for ext, params in ((".png", None), (".jpg", [ic.IMWRITE_JPEG_OPTIMIZE, 1]), (".jpg", [ic.IMWRITE_JPEG_PROGRESSIVE, 1]), (".jpg", [ic.IMWRITE_JPEG_QUALITY]),
                        (".jpg", [ic.IMWRITE_JPEG_SAMPLING_FACTOR, 0x411111]), (".jpg", [99, 1])):
        with pytest.raises(ValueError):
            ic.imencode(ext, img, params, ctx=ctx)
    with pytest.raises(ValueError):
        ic.imwrite(str(tmp_path / "out.png"), img, ctx=ctx)
    with pytest.raises(ValueError):
        ic.imencode(".jpg", img.astype(np.float32), ctx=ctx)


def test_recognize_stream_encode(ctx, monkeypatch):
    import cnn_oracle
    import constraint_ref as cr
    import test_gpu_propagate as tp
    from sudoku_vision_amd import Context, pipeline
    from sudoku_vision_amd.synth import synth_frames
    f0 = synth_frames(1, 270, 480, seed=11, device="cpu")[0][0].numpy()
    sd = cnn_oracle.random_state_dict(1234)
    given = np.array(cr.SELFTEST, np.uint8).reshape(81)
    tp._inject(monkeypatch, ctx, _dev(ctx, tp._logits(given))[None])
    with pytest.raises(ValueError):
        next(pipeline.recognize_stream([f0], sd, ctx=ctx, encode=True))
    base = list(pipeline.recognize_stream([f0] * 5, sd, ctx=ctx, glue=Context.GLUE_NORMALIZE, overlay=True))
    got = list(pipeline.recognize_stream([f0] * 5, sd, ctx=ctx, glue=Context.GLUE_NORMALIZE, overlay=True, encode=True))
    assert len(got) == 5 and any(r["solve_result"] == 1 for r in got)
    for r, b in zip(got, base):
        assert set(r) - set(b) == {"jpeg"} and isinstance(r["jpeg"], bytes)
        assert (r["frame_out"] == b["frame_out"]).all()
        drawn = r["frame_out"].cpu().numpy()
        assert r["jpeg"] == R.pillow_encode(drawn, 95, "420")
        assert (_pil_bgr(r["jpeg"]) == _pil_bgr(R.pillow_encode(drawn, 95, "420"))).all()
    assert any((r["frame_out"].cpu().numpy() != f0).any() for r in got)


def test_forward_entries_refuse_bad_arguments(ctx):
    """sv_jpeg_forward_bgr_u8 / _gray_u8 with a real context, plan and frame: every argument check of its own answers SV_ERR_BAD_ARG, and the
    good call next to it SV_OK."""
    from sudoku_vision_amd import _native
    H, W, BAD = 24, 40, -1
    lib, s = ctx._lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for ch, fn, other in ((3, lib.sv_jpeg_forward_bgr_u8, lib.sv_jpeg_forward_gray_u8), (1, lib.sv_jpeg_forward_gray_u8, lib.sv_jpeg_forward_bgr_u8)):
        plan = ctx.jpeg_encode_plan(W, H, ch, 75, "420", 0)
        ncoef, nb, row = int(plan.info.coef_count), int(plan.info.coef_count) // 64, ch * W
        frames = torch.zeros((2, H, row), dtype=torch.uint8, device=ctx.device)
        coef = torch.zeros((2, ncoef), dtype=torch.int16, device=ctx.device)
        masks = torch.zeros((2, nb), dtype=torch.int64, device=ctx.device)
        offsets = torch.zeros((2, nb), dtype=torch.int32, device=ctx.device)
        values = torch.zeros((2, ncoef), dtype=torch.int16, device=ctx.device)
        counts = torch.zeros((2,), dtype=torch.int32, device=ctx.device)
        f, c, m, o, v, k = (t.data_ptr() for t in (frames, coef, masks, offsets, values, counts))

        def call(fn=fn, plan=plan, src=f, n=2, pitch=row, stride=H * row, coef=c, masks=m, offsets=o, values=v, counts=k, h=ctx._h):
            return fn(h, C.byref(plan), src, n, pitch, stride, coef, masks, offsets, values, counts, s)
        assert call() == 0 and call(coef=None) == 0 and call(masks=None, offsets=None, values=None, counts=None) == 0
        assert call(n=1, stride=0) == 0                                # one frame: the stride is not looked at
        assert call(pitch=row - 1) == BAD and b"pitch" in lib.sv_last_error()
        assert call(stride=H * row - 1) == BAD                         # frames that overlap
        assert call(fn=other) == BAD and b"component" in lib.sv_last_error()      # a plan of the other entry
        assert call(counts=None) == BAD and b"together" in lib.sv_last_error()    # masks without counts
        assert call(masks=None) == BAD and call(offsets=None) == BAD and call(values=None) == BAD
        assert call(coef=None, masks=None, offsets=None, values=None, counts=None) == BAD and b"no output" in lib.sv_last_error()
        assert call(n=0) == BAD and call(n=-1) == BAD and call(n=65536) == BAD
        assert call(src=None) == BAD and call(h=None) == BAD and fn(ctx._h, None, f, 2, row, H * row, c, m, o, v, k, s) == BAD
        assert call(coef=c + 2) == BAD and call(masks=m + 4) == BAD and call(values=v + 1) == BAD      # misaligned outputs
        for edit in ("quality", "quant", "recip", "coef_count", "width", "orientation", "out_height", "h_samp"):
            bad = _native.JpegEnc.from_buffer_copy(plan)               # a plan is only what sv_jpeg_encode_plan makes
            if edit == "quality":
                bad.quality = 76
            elif edit in ("quant", "recip"):
                getattr(bad, edit)[70] += 1
            elif edit == "h_samp":
                bad.info.h_samp, bad.info.v_samp = 2, 2 if ch == 1 else 3
            else:
                setattr(bad.info, edit, getattr(bad.info, edit) + 1)
            assert call(plan=bad) == BAD, edit
        assert call() == 0
    torch.cuda.synchronize()


def test_run_pipeline_output(ctx, tmp_path, monkeypatch):
    """run.py --output: the solved frame, drawn on the GPU, is the file Pillow writes of the same pixels; a path this encoder does not write is
    reported, not raised."""
    import cnn_oracle
    import constraint_ref as cr
    from sudoku_vision_amd import host, imgcodecs, pipeline
    from sudoku_vision_amd.synth import synth_frames
    f0 = synth_frames(1, 270, 480, seed=11, device="cpu")[0][0].numpy()
    src = str(tmp_path / "in.jpg")
    Image.fromarray(np.ascontiguousarray(f0[..., ::-1]), "RGB").save(src, "JPEG", quality=95, subsampling=0)
    given = np.array(cr.SELFTEST, np.uint8).reshape(81)

    def reads_given(cells, want_digits=False, **kw):                   # the recogniser handed a solvable grid
        return None, torch.from_numpy(given).to(ctx.device), torch.ones(81, device=ctx.device)
    monkeypatch.setattr(ctx, "cnn_forward", reads_given)
    sd = cnn_oracle.random_state_dict(1234)
    plain = pipeline.run_pipeline(src, sd, ctx=ctx)
    assert plain.success and not hasattr(plain, "output_written")
    out = str(tmp_path / "solved.jpg")
    res = pipeline.run_pipeline(src, sd, ctx=ctx, output=out)
    assert res.success and res.error is None and res.output_written is True and res.solution == plain.solution
    frame = imgcodecs.imread(src, device=True, ctx=ctx)
    corners = host.find_grid_corners(ctx.preprocess(frame[None])[0].cpu().numpy())
    drawn = pipeline._draw_solution(ctx, frame[None], corners, given, np.asarray(res.solution, np.uint8).reshape(81), True)[0].cpu().numpy()
    assert (drawn != frame.cpu().numpy()).any()
    assert open(out, "rb").read() == R.pillow_encode(drawn, 95, "420")
    for bad in (str(tmp_path / "solved.png"), str(tmp_path / "no_such_dir" / "solved.jpg")):
        res = pipeline.run_pipeline(src, sd, ctx=ctx, output=bad)
        assert res.success and res.output_written is False and res.error.startswith("Output failed:") and res.solution == plain.solution
        assert not os.path.exists(bad)
    # an unsolved puzzle writes nothing
    clash = given.copy()
    clash[0], clash[1] = 5, 5
    monkeypatch.setattr(ctx, "cnn_forward", lambda cells, **kw: (None, torch.from_numpy(clash).to(ctx.device), torch.ones(81, device=ctx.device)))
    unsolved = str(tmp_path / "unsolved.jpg")
    res = pipeline.run_pipeline(src, sd, ctx=ctx, output=unsolved)
    assert not res.success and not hasattr(res, "output_written") and not os.path.exists(unsolved)
