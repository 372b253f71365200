"""GPU (-m gpu): the PNG encoder (csrc/k18_png_encode.hip + csrc/host_png.cpp; Context.imencode_png, imencode_png_batch, png_deflate,
imgcodecs.imencode_png / imwrite_png, recognize_stream(encode="png")).  Every file is checked four ways (check): Pillow decodes it to exactly the
input, in the right mode and size; zlib.decompress of its IDAT is the restatement's filtered bytes (tests/png_encode_ref.py: that pins the filter
bytes and the adaptive choice); the chunk layout and CRCs verify; and it is no larger than stored blocks would be."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import png_encode_ref as R

pytestmark = pytest.mark.gpu

SIZE_RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "png_encode_size.json")


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _same(a, b):
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and torch.equal(a, b)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if dataclasses.is_dataclass(a):
        return type(a) is type(b) and _same(vars(a), vars(b))
    return a == b


def check(ctx, img, filter="sub", strategy="rle", band_rows=0):
    """encode twice; all of the module docstring's checks; returns the file"""
    img = np.asarray(img)
    frame = _dev(ctx, img)
    data = ctx.imencode_png(frame, filter, strategy, band_rows=band_rows)
    what = (img.shape, filter, strategy, band_rows)
    assert isinstance(data, bytes) and data == ctx.imencode_png(frame, filter, strategy, band_rows=band_rows), what
    got, mode, size = R.pillow_decode(data)
    assert mode == ("L" if img.ndim == 2 else "RGB") and size == (img.shape[1], img.shape[0]), what
    assert (got == img).all(), what
    assert R.check_file(data, img) == R.filtered(img, filter), what
    plan = ctx.png_encode_plan(img.shape[1], img.shape[0], 1 if img.ndim == 2 else 3, filter, strategy, band_rows)
    raw = int(plan.filtered_bytes)
    assert len(data) <= raw + 5 * -(-raw // 65535) + 5 * int(plan.bands) + 64, what
    assert ctx.imencode_png_batch(frame[None], filter, strategy, band_rows=band_rows) == [data], what
    return data


def test_smallest_images(ctx):
    check(ctx, np.array([[7]], np.uint8))
    check(ctx, np.array([[[1, 2, 3]]], np.uint8))
    check(ctx, np.array([[0]], np.uint8))
    check(ctx, np.arange(5, dtype=np.uint8).reshape(5, 1) * 50)          # W = 1 gray, H = 5
    check(ctx, np.arange(5, dtype=np.uint8).reshape(5, 1) * 50, band_rows=2)


@pytest.mark.parametrize("mode", R.FILTERS)
def test_every_filter_mode(ctx, mode):
    check(ctx, R.content("synthetic", 5, 7), mode)                      # 7 x 5 BGR
    check(ctx, R.content("noise", 5, 7), mode)
    check(ctx, R.content("synthetic", 5, 7, gray=True), mode)
    check(ctx, R.content("synthetic", 48, 80), mode)


@pytest.mark.parametrize("run", [2, 3, 4, 258, 259, 260, 261, 517])
def test_runs_of_equal_filtered_bytes(ctx, run):
    """A gray row under the None filter whose filtered bytes hold a run of exactly `run` equal bytes between two other values: one literal, then
    matches of min(258, rest) while the rest is at least 3, then literals -- 2: no match; 3: no match (2 follow the literal); 4: one match of 3;
    259: one of 258; 260: 258 + 1 literal; 261: 258 + 2 literals; 517: 258 + 258."""
    row = np.concatenate([[9, 200], np.full(run, 41), [200, 9, 9, 41, 200]]).astype(np.uint8)
    f = R.filtered(row[None], "none")
    assert f == bytes([0]) + row.tobytes()
    a = check(ctx, row[None], "none")
    # under Sub the run of filtered bytes is the zeros after the run's first pixel
    check(ctx, row[None], "sub")
    # the same run ending the band, and starting it (behind the filter byte 0: a run of run + 1 zeros when the value is 0)
    check(ctx, np.concatenate([[9], np.full(run, 41)]).astype(np.uint8)[None], "none")
    check(ctx, np.zeros((1, run), np.uint8), "none")
    # matches shorten the file
    if run >= 258:
        assert len(a) < len(row) + 65


def test_all_zero_image(ctx):
    """64 x 48 zeros: every token but the first literal is a match, and the literal alphabet has two symbols (0 and end of block)"""
    for gray in (True, False):
        data = check(ctx, R.content("zeros", 48, 64, gray))
        assert len(data) < 65 + 250
    check(ctx, R.content("zeros", 48, 64, True), "none", band_rows=7)


def test_random_image_falls_back_to_stored_blocks(ctx):
    """53 x 37 uniformly random BGR: no matches (the distance code is declared all the same), and no Huffman code helps: stored blocks"""
    img = R.content("noise", 37, 53)
    data = check(ctx, img)
    raw = 37 * (1 + 3 * 53)
    assert len(data) == raw + 5 + 65                                     # one band, one stored block, the container
    check(ctx, img, "none", "huffman_only")
    check(ctx, img, band_rows=5)
    # a little structure: coded, with few or no matches
    check(ctx, (img // 16) * 16)
    check(ctx, (img // 16) * 16, "none", "huffman_only")


def test_flat_colour_wide(ctx):
    """1920 x 4 of one colour: under None the three channel bytes alternate (no run at all); under Sub every row is one literal pixel and a run that
    crosses the row's end up to the next filter byte; under Up the rows after the first are runs across row ends, filter byte aside"""
    img = R.content("flat", 4, 1920)
    for mode in ("none", "sub", "up", "adaptive"):
        check(ctx, img, mode)
    assert len(check(ctx, img, "sub")) < 65 + 400
    check(ctx, R.content("flat", 4, 1920, gray=True), "sub", band_rows=1)
    check(ctx, np.zeros((4, 1920), np.uint8), "none")                  # one run over all four rows, filter bytes included


@pytest.mark.parametrize("band_rows", [1, 3, 48])
def test_band_seams(ctx, band_rows):
    """80 x 48 synthetic: Up, Average and Paeth read the row above a band's first row from the image, not from the band"""
    img = R.content("synthetic", 48, 80)
    files = {mode: check(ctx, img, mode, band_rows=band_rows) for mode in R.FILTERS}
    plan = ctx.png_encode_plan(80, 48, 3, "sub", "rle", band_rows)
    assert plan.band_rows == band_rows and plan.bands == -(-48 // band_rows)
    assert len(set(files.values())) == 6
    check(ctx, R.content("synthetic", 48, 80, gray=True), "paeth", band_rows=band_rows)


def test_pitch_batch_and_views(ctx):
    H, W = 33, 41
    img = R.content("synthetic", H, W)
    want = check(ctx, img)
    buf = torch.zeros((H, 3 * W + 13), dtype=torch.uint8, device=ctx.device)
    buf[:, :3 * W] = _dev(ctx, img).view(H, 3 * W)
    pitched = buf[:, :3 * W].unflatten(1, (W, 3))
    assert pitched.stride() == (3 * W + 13, 3, 1) and not pitched.is_contiguous()
    assert ctx.imencode_png(pitched) == want                           # read in place by its pitch
    wide = _dev(ctx, np.repeat(img, 2, axis=1))
    assert ctx.imencode_png(wide[:, ::2]) == want                      # a non-contiguous view whose rows are not dense: packed first
    assert ctx.imencode_png(_dev(ctx, img[:, ::-1]).flip(1)) == want
    # n = 3 with a frame stride: frames cut out of a taller buffer
    imgs = [R.content(kind, H, W) for kind in ("synthetic", "noise", "zeros")]
    singles = [check(ctx, i, "adaptive", band_rows=4) for i in imgs]
    tall = torch.zeros((3, H + 5, W, 3), dtype=torch.uint8, device=ctx.device)
    for k, i in enumerate(imgs):
        tall[k, :H] = _dev(ctx, i)
    strided = tall[:, :H]
    assert not strided.is_contiguous()
    assert ctx.imencode_png_batch(strided, "adaptive", band_rows=4) == singles
    assert ctx.imencode_png_batch([_dev(ctx, i) for i in imgs], "adaptive", threads=4, band_rows=4) == singles
    old = ctx._ENC_CHUNK_BYTES
    try:
        ctx._ENC_CHUNK_BYTES = 1                                       # one frame per chunk
        assert ctx.imencode_png_batch(strided, "adaptive", threads=2, band_rows=4) == singles
    finally:
        ctx._ENC_CHUNK_BYTES = old
    gbuf = torch.zeros((H, W + 7), dtype=torch.uint8, device=ctx.device)
    gbuf[:, :W] = _dev(ctx, img[..., 1])
    assert ctx.imencode_png(gbuf[:, :W]) == check(ctx, img[..., 1])
    with pytest.raises(TypeError):
        ctx.imencode_png(img)                                           # a numpy array is imgcodecs.imencode_png's business
    with pytest.raises(ValueError):
        ctx.imencode_png_batch([_dev(ctx, imgs[0]), _dev(ctx, imgs[1])[:-8]])
    for bad in ({"filter": "best"}, {"strategy": "default"}, {"band_rows": -1}):
        with pytest.raises(ValueError):
            ctx.imencode_png(_dev(ctx, img), **bad)


def test_device_half_alone(ctx):
    """png_deflate: the bands back to back, their lengths, Adler sums and statuses; every band inflates on its own to its rows' filtered bytes"""
    import zlib
    img = R.content("synthetic", 48, 80)
    plan = ctx.png_encode_plan(80, 48, 3, "paeth", "rle", 5)
    stream, lens, adlers, status = (t.cpu().numpy() for t in ctx.png_deflate(_dev(ctx, img)[None], plan))
    assert stream.shape == (1, plan.stream_bound) and lens.shape == adlers.shape == status.shape == (1, 10) and not status.any()
    f = R.filtered(img, "paeth")
    per, at = 5 * plan.row_bytes, 0
    for b in range(10):
        piece = f[b * per:(b + 1) * per]
        n = int(lens[0, b])
        assert 5 <= n <= len(piece) + 5
        d = zlib.decompressobj(-15)
        assert d.decompress(stream[0, at:at + n].tobytes()) == piece and not d.eof and d.unused_data == b""
        assert stream[0, at + n - 4:at + n].tobytes() == b"\x00\x00\xff\xff" or n == len(piece) + 5       # coded bands end in the empty stored block
        assert int(adlers.view(np.uint32)[0, b]) == zlib.adler32(piece)
        at += n


def test_imgcodecs_names_and_parameters(ctx, tmp_path):
    from sudoku_vision_amd import imgcodecs as ic
    assert (ic.IMWRITE_PNG_COMPRESSION, ic.IMWRITE_PNG_STRATEGY, ic.IMWRITE_PNG_BILEVEL) == (16, 17, 18)
    assert (ic.IMWRITE_PNG_STRATEGY_DEFAULT, ic.IMWRITE_PNG_STRATEGY_FILTERED, ic.IMWRITE_PNG_STRATEGY_HUFFMAN_ONLY, ic.IMWRITE_PNG_STRATEGY_RLE,
            ic.IMWRITE_PNG_STRATEGY_FIXED) == (0, 1, 2, 3, 4)
    img = R.content("synthetic", 48, 80)
    frame = _dev(ctx, img)
    ok, buf = ic.imencode_png(img, ctx=ctx)                            # numpy in; Sub + RLE when the caller says nothing
    assert ok is True and buf.dtype == np.uint8 and buf.ndim == 1 and buf.tobytes() == ctx.imencode_png(frame, "sub", "rle")
    assert ic.imencode_png(frame, ctx=ctx)[1].tobytes() == buf.tobytes()
    assert ic.imencode_png(frame, [], ctx=ctx)[1].tobytes() == buf.tobytes()
    # HUFFMAN_ONLY
    data = ic.imencode_png(frame, [ic.IMWRITE_PNG_STRATEGY, ic.IMWRITE_PNG_STRATEGY_HUFFMAN_ONLY], ctx=ctx)[1].tobytes()
    assert data == ctx.imencode_png(frame, "sub", "huffman_only") == check(ctx, img, "sub", "huffman_only")
    assert ic.imencode_png(frame, [ic.IMWRITE_PNG_STRATEGY, ic.IMWRITE_PNG_STRATEGY_RLE], ctx=ctx)[1].tobytes() == buf.tobytes()
    # COMPRESSION 0: stored blocks only, one per band
    data = ic.imencode_png(frame, [ic.IMWRITE_PNG_COMPRESSION, 0], ctx=ctx)[1].tobytes()
    assert data == check(ctx, img, "sub", "stored")
    plan = ctx.png_encode_plan(80, 48, 3, "sub", "stored")
    assert len(data) == plan.filtered_bytes + 5 * plan.bands + 65
    # COMPRESSION 1..9: the adaptive filter, and nothing else
    level = [ic.imencode_png(frame, [ic.IMWRITE_PNG_COMPRESSION, k], ctx=ctx)[1].tobytes() for k in (1, 6, 9)]
    assert level[0] == level[1] == level[2] == check(ctx, img, "adaptive", "rle")
    assert ic.imencode_png(frame, [ic.IMWRITE_PNG_COMPRESSION, 3, ic.IMWRITE_PNG_STRATEGY, ic.IMWRITE_PNG_STRATEGY_HUFFMAN_ONLY, ic.IMWRITE_PNG_BILEVEL, 0],
                           ctx=ctx)[1].tobytes() == ctx.imencode_png(frame, "adaptive", "huffman_only")
    # gray, [H,W,1], a file
    g = ic.imencode_png(img[..., :1], ctx=ctx)[1].tobytes()
    assert g == ic.imencode_png(img[..., 0], ctx=ctx)[1].tobytes() == check(ctx, img[..., 0])
    path = str(tmp_path / "out.png")
    assert ic.imwrite_png(path, frame, ctx=ctx) is True and open(path, "rb").read() == buf.tobytes()
    assert ic.imwrite_png(path, img, [ic.IMWRITE_PNG_COMPRESSION, 5], ctx=ctx, threads=2) is True and open(path, "rb").read() == level[0]
    assert ic.imwrite_png(str(tmp_path / "no_such_dir" / "out.png"), img, ctx=ctx) is False
    for params in ([ic.IMWRITE_PNG_STRATEGY, ic.IMWRITE_PNG_STRATEGY_DEFAULT], [ic.IMWRITE_PNG_STRATEGY, ic.IMWRITE_PNG_STRATEGY_FILTERED],
                   [ic.IMWRITE_PNG_STRATEGY, ic.IMWRITE_PNG_STRATEGY_FIXED], [ic.IMWRITE_PNG_STRATEGY, 9], [ic.IMWRITE_PNG_BILEVEL, 1], [99, 1],
                   [ic.IMWRITE_JPEG_QUALITY, 90], [ic.IMWRITE_PNG_COMPRESSION]):
        with pytest.raises(ValueError):
            ic.imencode_png(img, params, ctx=ctx)
    for bad in (img.astype(np.float32), img[..., :2], np.zeros((4, 4, 3, 1), np.uint8), frame.float()):
        with pytest.raises(ValueError):
            ic.imencode_png(bad, ctx=ctx)
    # routing .png through imencode / imwrite is a later change: today they refuse, as before
    with pytest.raises(ValueError):
        ic.imencode(".png", img, ctx=ctx)
    with pytest.raises(ValueError):
        ic.imwrite(str(tmp_path / "x.png"), img, ctx=ctx)
    assert not os.path.exists(str(tmp_path / "x.png"))


def test_recognize_stream_png(ctx, monkeypatch):
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
        next(pipeline.recognize_stream([f0], sd, ctx=ctx, encode="png"))
    base = list(pipeline.recognize_stream([f0] * 5, sd, ctx=ctx, glue=Context.GLUE_NORMALIZE, overlay=True))
    got = list(pipeline.recognize_stream([f0] * 5, sd, ctx=ctx, glue=Context.GLUE_NORMALIZE, overlay=True, encode="png"))
    assert len(got) == 5 and any(r["solve_result"] == 1 for r in got)
    for r, b in zip(got, base):
        assert set(r) - set(b) == {"png"} and isinstance(r["png"], bytes)
        for k in b:
            assert _same(r[k], b[k]), k
        drawn = r["frame_out"].cpu().numpy()
        assert (R.pillow_decode(r["png"])[0] == drawn).all()
        assert R.check_file(r["png"], drawn) == R.filtered(drawn, "sub")
    assert any((r["frame_out"].cpu().numpy() != f0).any() for r in got)


def test_deflate_entries_refuse_bad_arguments(ctx):
    """sv_png_deflate_bgr_u8 / _gray_u8 with a real context, plan and frames: every argument check answers SV_ERR_BAD_ARG, and the good call next
    to it SV_OK."""
    from sudoku_vision_amd import _native
    H, W, BAD = 24, 40, -1
    lib, s = ctx._lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for ch, fn, other in ((3, lib.sv_png_deflate_bgr_u8, lib.sv_png_deflate_gray_u8), (1, lib.sv_png_deflate_gray_u8, lib.sv_png_deflate_bgr_u8)):
        plan = ctx.png_encode_plan(W, H, ch, "sub", "rle", 5)
        row, bands = ch * W, int(plan.bands)
        frames = torch.zeros((2, H, row), dtype=torch.uint8, device=ctx.device)
        stream = torch.zeros((2, int(plan.stream_bound)), dtype=torch.uint8, device=ctx.device)
        lens, adlers, status = (torch.zeros((2, bands + 1), dtype=torch.int32, device=ctx.device) for _ in range(3))
        f, o, l, a, st = (t.data_ptr() for t in (frames, stream, lens, adlers, status))

        def call(fn=fn, plan=plan, src=f, n=2, pitch=row, stride=H * row, out=o, lens=l, adlers=a, status=st, h=ctx._h):
            return fn(h, C.byref(plan), src, n, pitch, stride, out, lens, adlers, status, s)
        assert call() == 0
        assert call(n=1, stride=0) == 0                                # one frame: the stride is not looked at
        assert call(pitch=row - 1) == BAD and b"pitch" in lib.sv_last_error()
        assert call(stride=H * row - 1) == BAD and b"overlap" in lib.sv_last_error()
        assert call(fn=other) == BAD and b"channel" in lib.sv_last_error()
        assert call(n=0) == BAD and call(n=-1) == BAD and call(n=65536) == BAD
        assert call(src=None) == BAD and call(h=None) == BAD and call(out=None) == BAD and call(lens=None) == BAD and call(adlers=None) == BAD and call(status=None) == BAD
        assert fn(ctx._h, None, f, 2, row, H * row, o, l, a, st, s) == BAD
        assert call(lens=l + 2) == BAD and call(adlers=a + 1) == BAD and call(status=st + 3) == BAD and b"misaligned" in lib.sv_last_error()
        for edit in ("width", "height", "channels", "filter", "strategy", "band_rows", "bands", "row_bytes", "filtered_bytes", "slot_bytes", "stream_bound", "out_bound"):
            bad = _native.PngEnc.from_buffer_copy(plan)                # a plan is only what sv_png_encode_plan makes
            setattr(bad, edit, getattr(bad, edit) + (7 if edit in ("filter", "strategy") else 1))
            assert call(plan=bad) == BAD, edit
        assert call() == 0
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def size_record():
    with open(SIZE_RECORD) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["synthetic", "sample_1.jpg", "sample_4.jpg"])
def test_1080p_size_against_zlib_rle(ctx, size_record, name):
    """One 1080p frame with the default parameters against len(zlib_rle(filtered)), zlib at cv2's defaults.  The ratio is deterministic; it was
    measured once on an MI355X (profiles/png_encode_size.json, tools/time_png_encode.py --sizes) and may not grow past that by more than 0.02: the
    constant block header of about 150 bytes per band of 34 KB (0.5 %) and one Huffman code per band where zlib starts a new one every 16 k
    symbols.  More than 10 % over zlib is a defect whatever was recorded."""
    img = R.content("synthetic", 1080, 1920) if name == "synthetic" else R.photo_1080p(name)
    data = check(ctx, img)
    ratio = len(data) / len(R.zlib_rle(R.filtered(img, "sub")))
    print(f"{name}: {len(data)} bytes, ratio to zlib_rle {ratio:.4f}, recorded {size_record[name]['ratio']:.4f}")
    assert ratio <= 1.10
    assert ratio <= size_record[name]["ratio"] + 0.02
