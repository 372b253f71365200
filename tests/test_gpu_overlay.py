"""GPU: K16 (csrc/k16_overlay.hip) through Context.render_overlay == the numpy restatement (tests/overlay_ref.py), every byte of the
whole frame, at the GEOMETRIES; then the layers above it: resolve/overlay.py, recognize_image(overlay=True) and
recognize_stream(overlay=True)."""
import os
import sys

import numpy as np
import pytest
import torch

import constraint_ref as cr
import overlay_ref as ov
import warp_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_GEOMETRIES = [g for g in ov.GEOMETRIES if g.device]


@pytest.fixture(scope="module")
def atlas_ctx():
    """Contexts by atlas name: the session's (default glyphs, set lazily) and one of its own per custom atlas."""
    import sudoku_vision_amd as sva
    made = {}

    def get(name):
        if name == "font":
            return sva.default_context()
        if name not in made:
            made[name] = sva.Context()
            made[name].set_overlay_glyphs(ov.ATLASES[name]())
        return made[name]
    yield get
    for c in made.values():
        c.close()


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere((got != want).any(-1))
        y, x = bad[0][-2:]
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first at (x={x}, y={y}): got {got[tuple(bad[0])].tolist()} want {want[tuple(bad[0])].tolist()}")


def _args(ctx, g):
    digits, classes = ov.cells_of(g)
    return dict(m_dev=_dev(ctx, g.M[None]), digits=_dev(ctx, digits[None]), classes=_dev(ctx, classes[None]),
                palette=None if g.k == 3 else _dev(ctx, ov.palette_of(g)), shadow=g.shadow)


@pytest.fixture(scope="module")
def references():
    return {g.name: ov.reference(g) for g in DEVICE_GEOMETRIES}


@pytest.mark.parametrize("g", DEVICE_GEOMETRIES, ids=lambda g: g.name)
def test_geometry_out_of_place_and_in_place(atlas_ctx, references, g):
    ctx = atlas_ctx(g.atlas)
    frame = ov.frame_of(g)
    src = _dev(ctx, frame[None])
    out = ctx.render_overlay(src, **_args(ctx, g))
    _same(out[0], references[g.name], g.name)
    _same(src[0], frame, g.name + ": the source of an out-of-place call")
    assert ctx.render_overlay(src, out=src, **_args(ctx, g)) is src
    _same(src[0], references[g.name], g.name + " in place")


def test_shadow_switch_and_default_classes(ctx):
    g = ov.BY_NAME["persp_480x640"]
    digits, classes = ov.cells_of(g)
    frame = ov.frame_of(g)
    for shadow in (True, False):
        out = ctx.render_overlay(_dev(ctx, frame[None]), _dev(ctx, g.M[None]), _dev(ctx, digits[None]), shadow=shadow)
        _same(out[0], ov.render(frame, g.M, digits, None, None, ov.font_atlas(), shadow), f"classes=None, shadow={shadow}")
    one = _dev(ctx, ov.DEFAULT_PALETTE[:1])                 # k = 1: every cell of class 1 or 2 is not drawn
    out = ctx.render_overlay(_dev(ctx, frame[None]), _dev(ctx, g.M[None]), _dev(ctx, digits[None]), _dev(ctx, classes[None]), palette=one)
    _same(out[0], ov.render(frame, g.M, digits, classes, ov.DEFAULT_PALETTE[:1], ov.font_atlas()), "k = 1")


def test_cropped_view_is_drawn_in_place_and_nothing_else_is_touched(ctx):
    g = ov.Geometry("crop_200x256", "a view cropped out of a larger tensor", 200, 256, warp_ref._quad(130, 95, 90, 84, 11))
    digits, classes = ov.cells_of(g)
    rs = np.random.RandomState(g.seed)
    big = rs.randint(0, 256, (1, 260, 300, 3), dtype=np.uint8)
    view_np = big[0, 31:231, 17:273]
    want = ov.render(view_np, g.M, digits, classes, None, ov.font_atlas())
    args = dict(m_dev=_dev(ctx, g.M[None]), digits=_dev(ctx, digits[None]), classes=_dev(ctx, classes[None]))
    # out of place from the view: pitch > 3 W on the source side only
    src = _dev(ctx, big)
    _same(ctx.render_overlay(src[:, 31:231, 17:273], **args)[0], want, "from a cropped view")
    _same(src, big, "the source tensor")
    # into a view of another tensor, and in place in the view
    dst = _dev(ctx, big[:, ::-1].copy())
    ctx.render_overlay(src[:, 31:231, 17:273], out=dst[:, 31:231, 17:273], **args)
    expect = big[:, ::-1].copy()
    expect[0, 31:231, 17:273] = want
    _same(dst, expect, "into a cropped view")
    view = src[:, 31:231, 17:273]
    assert ctx.render_overlay(view, out=view, **args) is view
    expect = big.copy()
    expect[0, 31:231, 17:273] = want
    _same(src, expect, "in place in a cropped view")


def test_three_frames_with_the_middle_one_inactive(ctx):
    gs = [ov.Geometry(f"batch_{i}", "", 70, 100, c) for i, c in enumerate(
        (warp_ref._quad(50, 35, 30, 28, 5), warp_ref._quad(45, 30, 33, 30, -12), np.array([[5, 3], [90, 8], [96, 66], [2, 60]], np.float32)))]
    frames = np.stack([ov.frame_of(g) for g in gs])
    cells = [ov.cells_of(g) for g in gs]
    digits = np.stack([c[0] for c in cells])
    digits[2] = np.roll(digits[2], 7)
    classes = np.stack([c[1] for c in cells])
    M = np.stack([g.M for g in gs])
    want = np.stack([ov.render(frames[i], M[i], digits[i], classes[i], None, ov.font_atlas()) for i in range(3)])
    want[1] = frames[1]
    for active in (torch.tensor([1, 0, 1], dtype=torch.uint8, device=ctx.device), torch.tensor([True, False, True], device=ctx.device)):
        src = _dev(ctx, frames)
        out = ctx.render_overlay(src, _dev(ctx, M), _dev(ctx, digits), _dev(ctx, classes), active=active)
        _same(out, want, "n = 3, out of place")
        ctx.render_overlay(src, _dev(ctx, M), _dev(ctx, digits), _dev(ctx, classes), active=active, out=src)
        _same(src, want, "n = 3, in place")


def test_small_quad_in_a_1080p_frame_in_place(ctx):
    H, W = 1080, 1920
    corners = np.array([[1203, 411], [1342, 420], [1335, 560], [1198, 548]], np.float32)
    g = ov.Geometry("small_in_1080p", "", H, W, corners)
    digits, classes = ov.cells_of(g)
    frame = ov.frame_of(g)
    src = _dev(ctx, frame[None])
    ctx.render_overlay(src, _dev(ctx, g.M[None]), _dev(ctx, digits[None]), _dev(ctx, classes[None]), out=src)
    got = src[0].cpu().numpy()
    x0, y0 = np.floor(corners.min(0)).astype(int)
    x1, y1 = np.ceil(corners.max(0)).astype(int)
    outside = np.ones((H, W), bool)
    outside[y0:y1 + 1, x0:x1 + 1] = False
    assert (got[outside] == frame[outside]).all()
    _same(got, ov.render(frame, g.M, digits, classes, None, ov.font_atlas()), g.name)
    assert (got != frame).any()


def test_atlas_with_a_margin_texel_is_refused(atlas_ctx):
    import sudoku_vision_amd as sva
    ctx = atlas_ctx("full")
    bad = ov.full_atlas()
    bad[8, 47, 30] = 200
    with pytest.raises(sva._native.NativeError, match="SV_ERR_BAD_ARG.*glyph 8.*row 47, column 30"):
        ctx.set_overlay_glyphs(bad)
    with pytest.raises(ValueError):
        ctx.set_overlay_glyphs(bad[:8])
    with pytest.raises(ValueError):
        ctx.set_overlay_glyphs(bad.astype(np.int32))
    g = ov.BY_NAME["full_atlas"]                            # the refused atlas replaced nothing
    _same(ctx.render_overlay(_dev(ctx, ov.frame_of(g)[None]), **_args(ctx, g))[0], ov.reference(g), "after a refused atlas")


def test_render_overlay_argument_checks(ctx):
    g = ov.BY_NAME["odd_37x53"]
    a = _args(ctx, g)
    frames = _dev(ctx, ov.frame_of(g)[None])
    with pytest.raises(TypeError):
        ctx.render_overlay(frames.cpu(), **a)
    with pytest.raises(TypeError):
        ctx.render_overlay(frames.to(torch.int32), **a)
    with pytest.raises(ValueError):
        ctx.render_overlay(frames[0], **a)
    with pytest.raises(ValueError):
        ctx.render_overlay(frames[..., :2], **a)
    with pytest.raises(TypeError):
        ctx.render_overlay(frames, **{**a, "m_dev": a["m_dev"].float()})
    with pytest.raises(ValueError):
        ctx.render_overlay(frames, **{**a, "m_dev": a["m_dev"].reshape(9)[:8]})
    with pytest.raises(ValueError):
        ctx.render_overlay(frames, **{**a, "digits": a["digits"][:, :80]})
    with pytest.raises(TypeError):
        ctx.render_overlay(frames, **{**a, "digits": a["digits"].to(torch.int64)})
    with pytest.raises(ValueError):
        ctx.render_overlay(frames, **{**a, "classes": a["classes"].reshape(81)})
    with pytest.raises(ValueError):
        ctx.render_overlay(frames, **{**a, "palette": torch.zeros((3, 4), dtype=torch.uint8, device=ctx.device)})
    with pytest.raises(ValueError):
        ctx.render_overlay(frames, active=torch.ones(2, dtype=torch.uint8, device=ctx.device), **a)
    with pytest.raises(ValueError):
        ctx.render_overlay(frames, out=torch.empty((1, 37, 54, 3), dtype=torch.uint8, device=ctx.device), **a)
    with pytest.raises(TypeError):
        ctx.render_overlay(frames, out=torch.empty((1, 37, 53, 3), dtype=torch.uint8), **a)


# ---- the layers above ------------------------------------------------------------------------------------------------------------
def _dropin():
    d = os.path.join(ROOT, "sudoku-vision_amd", "resolve")
    if d not in sys.path:
        sys.path.insert(0, d)
    import overlay
    return overlay


def _solved(given):
    from sudoku_vision_amd import host
    code, sol = host.solve_sudoku(np.asarray(given).reshape(9, 9).tolist())
    assert code == 1
    return np.asarray(sol, np.uint8).reshape(81)


def _drawn(frame, corners, given, solution):
    """The reference: the cells `given` leaves empty, drawn at `corners` through the library's own forward homography."""
    import sudoku_vision_amd as sva
    m, ok = sva.Context.corners_to_m_batch(np.asarray(corners, np.float32).reshape(1, 4, 2))
    assert ok[0]
    digits = np.where(np.asarray(given).reshape(81) != 0, 0, np.asarray(solution).reshape(81)).astype(np.uint8)
    return ov.render(frame, m[0], digits, None, None, ov.font_atlas())


def test_render_solution_on_frame(ctx):
    mod = _dropin()
    g = ov.BY_NAME["persp_480x640"]
    frame = ov.frame_of(g)
    given = np.array(cr.SELFTEST, np.uint8).reshape(81)
    sol = _solved(given)
    conf = np.random.RandomState(4).uniform(0.5, 1.0, 81)
    got = mod.render_solution_on_frame(frame, g.corners, given.reshape(9, 9).tolist(), sol.reshape(9, 9).tolist(), ctx=ctx)
    assert isinstance(got, np.ndarray)
    _same(got, _drawn(frame, g.corners, given, sol), "render_solution_on_frame")
    got = mod.render_solution_on_frame(_dev(ctx, frame), g.corners[[2, 0, 3, 1]], given, sol, conf, show_originals=True, shadow=False, ctx=ctx)
    assert isinstance(got, torch.Tensor)
    import sudoku_vision_amd as sva
    m, _ = sva.Context.corners_to_m_batch(g.corners[None])
    digits, classes = mod.overlay_cells(given, sol, conf, show_originals=True)
    assert set(classes.tolist()) == {0, 1, 2}
    _same(got, ov.render(frame, m[0], digits, classes, None, ov.font_atlas(), shadow=False), "show_originals")
    _same(mod.render_solution_on_frame(frame, np.zeros((4, 2), np.float32), given, sol, ctx=ctx), frame, "degenerate corners")


def test_recognize_image_overlay(ctx, monkeypatch):
    import cnn_oracle
    import test_gpu_propagate as tp
    from sudoku_vision_amd import Context, pipeline
    from sudoku_vision_amd.synth import synth_frames
    f0 = synth_frames(1, 270, 480, seed=11, device="cpu")[0][0].numpy()
    sd = cnn_oracle.random_state_dict(1234)
    with pytest.raises(ValueError):
        pipeline.recognize_image(f0, sd, ctx=ctx, overlay=True)
    given = np.array(cr.SELFTEST, np.uint8).reshape(81)
    tp._inject(monkeypatch, ctx, _dev(ctx, tp._logits(given))[None])
    base = pipeline.recognize_image(f0, sd, ctx=ctx, glue=Context.GLUE_NORMALIZE, solve=True)
    res = pipeline.recognize_image(f0, sd, ctx=ctx, glue=Context.GLUE_NORMALIZE, solve=True, overlay=True)
    assert set(res) - set(base) == {"overlay"} and res["solve_result"] == 1 and res["grid"] == cr.SELFTEST
    for key in base:
        assert np.array_equal(np.asarray(res[key], dtype=object), np.asarray(base[key], dtype=object)), key
    assert isinstance(res["overlay"], torch.Tensor) and res["overlay"].device == ctx.device
    _same(res["overlay"], _drawn(f0, res["corners"], res["grid"], res["solution"]), "recognize_image(overlay=True)")
    assert (res["overlay"].cpu().numpy() != f0).any()
    # an unsolvable reading: an unchanged copy
    clash = given.copy()
    clash[0], clash[1] = 5, 5
    tp._inject(monkeypatch, ctx, _dev(ctx, tp._logits(clash))[None])
    res = pipeline.recognize_image(f0, sd, ctx=ctx, glue=Context.GLUE_NORMALIZE, solve=True, overlay=True)
    assert res["solve_result"] != 1
    _same(res["overlay"], f0, "unsolved")


def test_recognize_stream_overlay(ctx, monkeypatch):
    import cnn_oracle
    import test_gpu_propagate as tp
    from sudoku_vision_amd import Context, pipeline
    from sudoku_vision_amd.synth import synth_frames
    f0 = synth_frames(1, 270, 480, seed=11, device="cpu")[0][0].numpy()
    sd = cnn_oracle.random_state_dict(1234)
    given = np.array(cr.SELFTEST, np.uint8).reshape(81)
    tp._inject(monkeypatch, ctx, _dev(ctx, tp._logits(given))[None])
    plain = list(pipeline.recognize_stream([f0] * 6, sd, ctx=ctx, glue=Context.GLUE_NORMALIZE))
    got = list(pipeline.recognize_stream([f0] * 6, sd, ctx=ctx, glue=Context.GLUE_NORMALIZE, overlay=True))
    assert len(got) == 6 and sum(r["corners_used"] is not None for r in got) >= 3
    sol = _solved(given)
    for r, p in zip(got, plain):
        assert set(r) - set(p) == {"solution", "solve_result", "frame_out"}
        assert r["motion"] == p["motion"] and r["detected"] == p["detected"] and (r["digits"] is None) == (p["digits"] is None)
        assert isinstance(r["frame_out"], torch.Tensor) and r["frame_out"].device == ctx.device
        if r["corners_used"] is None:
            assert r["solution"] is None and r["solve_result"] is None
            _same(r["frame_out"], f0, "a frame without corners")
        else:
            assert (r["digits"] == given).all() and (p["digits"] == given).all() and r["solve_result"] == 1 and (r["solution"] == sol).all()
            _same(r["frame_out"], _drawn(f0, r["corners_used"], given, sol), "recognize_stream(overlay=True)")
