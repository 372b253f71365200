"""The case table of tests/test_gpu_stream_order.py: one row per Context entry and variant.

A row holds two complete, valid inputs A and B (numpy, made here, giving different results), the call on device tensors that hold one of
them, and want(inputs): the CPU restatement the entry's own GPU test compares exactly against.  Nothing here needs a GPU: the module
imports without one and every want() runs on the host (tests/test_stream_cases_ref.py).

kind "pure": the entry never reads a device result on the host; it runs on a side stream behind a delay (Part 1) and is captured into a
graph and replayed on other contents (Part 3).  kind "host": its code synchronises or takes host bytes; Part 1 only.  kind "decode": the
input is the bytes of a file, A and B of different sizes, and three decodes A, B, A queue behind one delay (the staging ring).

want is None where the entry is compared against float64 under a tolerance rule by its own test (the CNN forwards, softmax_topk's
probabilities, cell_ink_ratio's ratio): the test then demands bit-equality with an eager, synchronised call on the default stream.

Keys of an input dict that start with "_" stay on the host (a file the buffers were made from); every other key is a device buffer that
never holds anything but A or B."""
import ctypes as C
import zlib

import numpy as np

import cnn_oracle
import component_filter_ref as cfr
import constraint_ref as cr
import despeckle_ref as dr
import grid_v2_ref as gr
import jpeg_craft
import jpeg_encode_ref as jer
import jpeg_gray_ref
import jpeg_reduced_ref
import model_v3_light_ref
import model_v3_ref
import overlay_ref
import png_craft
import png_decode_ref
import png_encode_ref as per
import preprocess_v2_ref as p2
import quality_ref
import resolve_ref as rr
import solve_ref as sr
import stabilizer_ref
import sv_oracle as o
import warp_ref

SMALL, LARGE = (2, 48, 64), (2, 96, 160)          # the frames of tests/test_gpu_scratch.py; W % 32 == 0 for the bit-image entries
U8, I32, F32, F64 = np.uint8, np.int32, np.float32, np.float64


class Case:
    def __init__(self, name, make, call, want=None, kind="pure", norm=None, xcheck=False):
        self.name, self.make, self.call, self.want, self.kind, self.norm, self.xcheck = name, make, call, want, kind, norm, xcheck
        self._ab = None

    def inputs(self):
        """(A, B), made once"""
        if self._ab is None:
            self._ab = (self.make(1), self.make(2))
        return self._ab


CASES = []


def case(name, make, call, want=None, **kw):
    CASES.append(Case(name, make, call, want, **kw))


def by_name(name):
    return next(c for c in CASES if c.name == name)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _noise(seed, shape, tag=0):
    return np.random.RandomState(1000 * tag + seed).randint(0, 256, shape).astype(U8)


def _smooth(seed, shape, tag=0):
    """noise over a ramp: a gray image with a background, so that the local-mean entries have something to find"""
    n, H, W = shape
    ramp = (np.arange(W)[None, None, :] * (120 + 40 * seed) // W + np.arange(H)[None, :, None] * 60 // H)
    return np.clip(ramp + _noise(seed, shape, tag) // 3, 0, 255).astype(U8)


def _bgr(shape):
    return lambda seed: {"frames": _noise(seed, shape + (3,))}


def _gray(shape, fn=_noise):
    return lambda seed: {"gray": fn(seed, shape)}


def _quads(seed, n, H, W):
    """n convex quads inside an H x W frame, different for every seed and frame"""
    rs = np.random.RandomState(77 + seed)
    j = lambda: rs.uniform(0, 0.12)
    return np.array([[[W * j(), H * j()], [W * (1 - j()), H * j()], [W * (1 - j()), H * (1 - j())], [W * j(), H * (1 - j())]] for _ in range(n)], F32)


def _minv(seed, n, H, W):
    """destination -> source maps of _quads onto the 450 square: what corners_to_minv gives, from warp_ref's own DLT"""
    return np.stack([np.linalg.inv(warp_ref.homography(q, 450)) for q in _quads(seed, n, H, W)])


def _bgr_minv(shape):
    return lambda seed: {"frames": _noise(seed, shape + (3,)), "minv": _minv(seed, shape[0], shape[1], shape[2])}


def _binary(seed, shape, density=0.45):
    return ((np.random.RandomState(500 + seed).rand(*shape) < density) * 255).astype(U8)


def _specks(seed, shape):
    """sparse dots and one outline that crosses the 64 x 64 tiles: every flood fill of the speck filter ends after a few steps"""
    n, H, W = shape
    img = ((np.random.RandomState(600 + seed).rand(*shape) < 0.02) * 255).astype(U8)
    for f in range(n):
        t, l = 4 + 2 * seed + f, 6 + 3 * seed
        img[f, t:H - 5, l:l + 2] = img[f, t:H - 5, W - 9:W - 7] = img[f, t:t + 2, l:W - 7] = img[f, H - 7:H - 5, l:W - 7] = 255
    return img


def _components(seed, shape):
    """components on both sides of the floor of 1 % of the frame: dots and short strokes, and two outlines that stay"""
    n, H, W = shape
    rs = np.random.RandomState(700 + seed)
    img = ((rs.rand(*shape) < 0.01) * 255).astype(U8)
    for f in range(n):
        for _ in range(6):
            y, x, ln = rs.randint(2, H - 30), rs.randint(2, W - 40), rs.randint(5, 30)
            img[f, y:y + ln, x] = 255
            img[f, y, x:x + ln] = 255
        t, l = 3 + seed + f, 5 + 2 * seed
        img[f, t:H - 4, l] = img[f, t:H - 4, W - 6] = img[f, t, l:W - 5] = img[f, H - 5, l:W - 5] = 255
    return img


# ---- K1, K2, K4, K6, K11, K13 ---------------------------------------------------------------------------------------------------------
def _per_frame(fn, x, *more):
    return np.stack([fn(*(a[f] for a in (x,) + more)) for f in range(len(x))])


case("gray", _bgr(SMALL), lambda c, d: (c.gray(d["frames"]),), lambda i: (_per_frame(o.gray, i["frames"]),))
case("blur", _gray(SMALL), lambda c, d: (c.blur(d["gray"], 5),), lambda i: (_per_frame(lambda g: o.gaussian_blur(g, 5), i["gray"]),))
case("adaptive_threshold", _gray(SMALL), lambda c, d: (c.adaptive_threshold(d["gray"], 11, 2, True),),
     lambda i: (_per_frame(lambda g: o.adaptive_threshold(g, 11, 2, True), i["gray"]),))
case("preprocess", _bgr(LARGE), lambda c, d: (c.preprocess(d["frames"]),), lambda i: (_per_frame(o.preprocess_for_grid_detection, i["frames"]),))
case("preprocess_bits", _bgr(LARGE), lambda c, d: (c.preprocess_bits(d["frames"]),),
     lambda i: (cfr.pack_bits(_per_frame(o.preprocess_for_grid_detection, i["frames"])),))
case("preprocess_mm+preprocess_stats", _bgr(SMALL), lambda c, d: (c.preprocess_mm(d["frames"]), np.array(c.preprocess_stats()[1])),
     lambda i: (_per_frame(o.preprocess_for_grid_detection, i["frames"]), np.array(0)), kind="host", xcheck=True)
case("preprocess_and_warp_cells", _bgr_minv(LARGE), lambda c, d: c.preprocess_and_warp_cells(d["frames"], d["minv"]),
     lambda i: (_per_frame(o.preprocess_for_grid_detection, i["frames"]), _per_frame(warp_ref.cells, i["frames"], i["minv"])))
case("warp_cells", _bgr_minv(SMALL), lambda c, d: (c.warp_cells(d["frames"], d["minv"]),),
     lambda i: (_per_frame(warp_ref.cells, i["frames"], i["minv"]),))
case("warp_perspective", lambda s: {"img": _noise(s, SMALL[1:] + (3,)), "minv": _minv(s, 1, *SMALL[1:])},
     lambda c, d: (c.warp_perspective(d["img"], d["minv"], 450),), lambda i: (warp_ref.warp(i["img"], i["minv"][0], 450),))
case("extract_cells", lambda s: {"grid": _noise(s, (450, 450))}, lambda c, d: (c.extract_cells(d["grid"], 28, 5, 5),),
     lambda i: (warp_ref.extract(i["grid"], 28, 0.1),))
case("resize_linear", lambda s: {"img": _noise(s, SMALL[1:])}, lambda c, d: (c.resize_linear(d["img"], (28, 28)),),
     lambda i: (o.resize_linear(i["img"], (28, 28)),))
case("warp_affine", lambda s: {"img": _noise(s, SMALL), "M": np.stack([gr.rotation_matrix((32, 24), 7.0 * s + 3 * f, 1.1) for f in range(2)]).astype(F64)},
     lambda c, d: (c.warp_affine(d["img"], d["M"], (72, 40), 255),),
     lambda i: (np.stack([gr.warp_affine(i["img"][f], i["M"][f], (72, 40), 255) for f in range(2)]),))


def _despeckled(img):
    want, hard, unsure = dr.despeckle(img)
    assert not hard and not unsure, "the input leaves a tile to the iteration cap"
    return (want * 255).astype(U8)


def _work(buf):
    """The in-place entries run on a copy, made on the current stream: the input buffer keeps A or B."""
    return buf.clone()


case("despeckle", lambda s: {"binary": _specks(s, LARGE)}, lambda c, d: (c.despeckle(d["binary"]),), lambda i: (_per_frame(_despeckled, i["binary"]),))
case("despeckle_bits", lambda s: {"bits": cfr.pack_bits(_specks(s, LARGE))}, lambda c, d: (c.despeckle_bits(_work(d["bits"])),),
     lambda i: (cfr.pack_bits(_per_frame(_despeckled, cfr.unpack_bits(i["bits"], LARGE[2]))),))
case("component_filter", lambda s: {"binary": _components(s, LARGE)}, lambda c, d: (c.component_filter(d["binary"], min_area_ratio=0.01),),
     lambda i: (_per_frame(lambda b: cfr.component_filter(b, 0.01), i["binary"]),))
case("component_filter_bits", lambda s: {"bits": cfr.pack_bits(_components(s, LARGE))},
     lambda c, d: (c.component_filter_bits(_work(d["bits"]), min_area_ratio=0.01),),
     lambda i: (cfr.pack_bits(_per_frame(lambda b: cfr.component_filter(b, 0.01), cfr.unpack_bits(i["bits"], LARGE[2]))),))


def _records_stride():
    from sudoku_vision_amd import host
    return host.sparse_bits_record_bytes(LARGE[1], LARGE[2], LARGE[1] * LARGE[2] // 32)


def _pack_sparse_call(c, d):
    import torch
    return (c.pack_sparse_bits(d["bits"], torch.zeros((LARGE[0], _records_stride()), dtype=torch.uint8, device=c.device)),)


def _pack_sparse_want(i):
    from sudoku_vision_amd import host
    from test_host_contours import _pack_sparse_np
    return (np.stack([_pack_sparse_np(host, b.view(np.uint32), LARGE[1] * LARGE[2] // 32) for b in i["bits"]]),)


case("pack_sparse_bits", lambda s: {"bits": cfr.pack_bits(_specks(s, LARGE))}, _pack_sparse_call, _pack_sparse_want)


def _quality_want(i):
    st = [quality_ref.frame_stats(f) for f in i["frames"]]
    return (np.array([s[0] for s in st], np.int64), np.array([s[1] for s in st], np.int64), np.stack([s[2] for s in st]).astype(I32))


case("frame_quality_stats", _bgr(SMALL), lambda c, d: c.frame_quality_stats(d["frames"]), _quality_want)
case("grid_line_coverage_u8", lambda s: {"binary": _binary(s, LARGE), "minv": _minv(s, 2, *LARGE[1:])},
     lambda c, d: (c.grid_line_coverage(d["binary"], d["minv"]),),
     lambda i: (_per_frame(warp_ref.band_counts, i["binary"], i["minv"]).astype(I32),))
case("grid_line_coverage_bits", lambda s: {"bits": cfr.pack_bits(_binary(s, LARGE)), "minv": _minv(s, 2, *LARGE[1:])},
     lambda c, d: (c.grid_line_coverage(d["bits"], d["minv"]),),
     lambda i: (_per_frame(warp_ref.band_counts, cfr.unpack_bits(i["bits"], LARGE[2]).astype(U8) * 255, i["minv"]).astype(I32),))


def _harris_call(c, d):
    corners, counts = c.harris_corners(d["gray"], max_corners=50, min_distance=3)
    return corners, counts


def _harris_norm(got, i):
    corners, counts = got
    corners = corners.copy()
    for f, n in enumerate(counts):
        corners[f, n:] = 0                                     # rows past a frame's count are not written
    return corners, counts


def _harris_want(i):
    per = [gr.harris_corners(g, 50, 0.01, 3)[0] for g in i["gray"]]
    corners = np.zeros((len(per), 50, 2), F32)
    for f, p in enumerate(per):
        corners[f, :len(p)] = p
    return corners, np.array([len(p) for p in per], I32)


case("harris_corners", _gray(SMALL, _smooth), _harris_call, _harris_want, kind="host", norm=_harris_norm)


# ---- K7 -------------------------------------------------------------------------------------------------------------------------
def _two(name, fn=_smooth):
    return lambda s: {"gray": fn(s, LARGE), name: fn(s, LARGE, tag=3)}


case("morphology_close_ellipse5", _gray(LARGE), lambda c, d: (c.morphology(d["gray"], c.MORPH_CLOSE, c.SHAPE_ELLIPSE, 5),),
     lambda i: (_per_frame(lambda g: p2.morph_close(g, p2.structuring_element("ellipse", 5)), i["gray"]),))
case("box_mean", _gray(LARGE), lambda c, d: (c.box_mean(d["gray"], 21),), lambda i: (_per_frame(lambda g: p2.box_mean(g, 21), i["gray"]),))
case("gaussian_blur21", _gray(LARGE), lambda c, d: (c.gaussian_blur21(d["gray"]),), lambda i: (_per_frame(p2.gaussian_blur21, i["gray"]),))
case("divide_normalize", _two("background"), lambda c, d: (c.divide_normalize(d["gray"], d["background"]),),
     lambda i: (_per_frame(p2.divide_normalize, i["gray"], i["background"]),))
case("clahe", _gray(LARGE, _smooth), lambda c, d: (c.clahe(d["gray"], 2.0, (8, 8)),), lambda i: (_per_frame(lambda g: p2.clahe(g, 2.0, (8, 8)), i["gray"]),))
case("threshold_sauvola", _gray(LARGE, _smooth), lambda c, d: (c.threshold_sauvola(d["gray"], 25, 0.2),),
     lambda i: (_per_frame(lambda g: p2.threshold_sauvola(g, 25, 0.2), i["gray"]),))
_threshold_call = lambda c, d: c.threshold_count(d["gray"], 100, False)
_threshold_want = lambda i: (((i["gray"] > 100) * 255).astype(U8), (i["gray"] > 100).sum((1, 2)).astype(I32))
_shadow_call = lambda c, d: c.shadow_mask(d["gray"], d["local_mean"], -30)
_shadow_want = lambda i: ((((i["gray"].astype(int) - i["local_mean"].astype(int)) < -30) * 255).astype(U8),
                          ((i["gray"].astype(int) - i["local_mean"].astype(int)) < -30).sum((1, 2)).astype(I32))
_nonzero_call = lambda c, d: (c.count_nonzero(d["gray"]),)
_nonzero_want = lambda i: ((i["gray"] != 0).sum((1, 2)).astype(I32),)
case("threshold_count", _gray(LARGE), _threshold_call, _threshold_want)
case("shadow_mask", _two("local_mean", _noise), _shadow_call, _shadow_want)
case("count_nonzero", lambda s: {"gray": _binary(s, LARGE, 0.3 + 0.1 * s)}, _nonzero_call, _nonzero_want)
# five frames: the per-frame counts are 20 bytes, past the 16 from which a captured hipMemsetAsync was not replayed
MANY = (5, 48, 64)
case("threshold_count_n5", _gray(MANY), _threshold_call, _threshold_want)
case("shadow_mask_n5", lambda s: {"gray": _noise(s, MANY), "local_mean": _noise(s, MANY, tag=3)}, _shadow_call, _shadow_want)
case("count_nonzero_n5", lambda s: {"gray": _binary(s, MANY, 0.3 + 0.1 * s)}, _nonzero_call, _nonzero_want)


# ---- cells and the CNN forwards (want None: bit-equality with an eager call) ---------------------------------------------------------
def _cells_u8(n=81):
    return lambda s: {"cells": _smooth(s, (n, 28, 28), tag=5)}


def _cells_f32(s):
    return {"x": model_v3_ref.inputs(40 + s, 81)}


case("cell_ink_ratio", _cells_u8(), lambda c, d: c.cell_ink_ratio(d["cells"]))
case("preprocess_cells", _cells_u8(), lambda c, d: (c.preprocess_cells(d["cells"]),), lambda i: (o.preprocess_cells(i["cells"]),))
case("softmax_topk", lambda s: {"logits": rr.real_logits(90 + s, 1).reshape(-1, 10).astype(F32)}, lambda c, d: c.softmax_topk(d["logits"], 3))


def _bf16(c, d):
    c.set_precision(c.PREC_BF16)
    try:
        return c.cnn_forward(d["cells"], want_digits=True)
    finally:
        c.set_precision(c.PREC_F32)


case("cnn_forward_f32", _cells_f32, lambda c, d: c.cnn_forward(d["x"], want_digits=True))
case("cnn_forward_u8", _cells_u8(), lambda c, d: c.cnn_forward(d["cells"], want_digits=True))
case("cnn_forward_u8_bf16", _cells_u8(), _bf16)
case("cnn3_forward", _cells_f32, lambda c, d: c.cnn3_forward(d["x"], want_digits=True, want_features=True))
case("cnn3_light_forward", _cells_f32, lambda c, d: c.cnn3_light_forward(d["x"], want_digits=True, want_features=True))
case("empty_forward", _cells_f32, lambda c, d: (c.empty_forward(d["x"]),))
for _name in ("frames_to_digits", "frames_to_digits_v3", "frames_to_digits_v3_light"):
    case(_name, _bgr_minv(LARGE),
         lambda c, d, _n=_name: (lambda r: (r["logits"], r["digits"], r["conf"], r["cells"]))(getattr(c, _n)(d["frames"], d["minv"], keep_cells=True)))


def load_weights(ctx):
    """every weight set the forwards need, once per context"""
    ctx.load_state_dict(cnn_oracle.random_state_dict(1234))
    ctx.load_state_dict_v3(model_v3_ref.random_state_dict_v3(2024, True))
    ctx.load_state_dict_v3_light(model_v3_light_ref.random_state_dict_light(7))
    ctx.load_state_dict_empty(model_v3_light_ref.random_state_dict_empty(8))


# ---- K9, K10, K14 ---------------------------------------------------------------------------------------------------------------
def _resolve_inputs(s):
    index, prob = rr.frames(rr.GOLDEN_SEED, 16)                 # the head of the golden set: frames with conflicts to repair among them
    return {"index": index[8 * (s - 1):8 * s][:2].copy(), "prob": prob[8 * (s - 1):8 * s][:2].copy()}


def _dict_call(method, fields, *keys, **kw):
    def call(c, d):
        r = getattr(c, method)(*(d[k] for k in keys), **kw)
        return tuple(r[f] for f in fields)
    return call


case("resolve_conflicts", _resolve_inputs, _dict_call("resolve_conflicts", rr.FIELDS, "index", "prob"),
     lambda i: (lambda r: tuple(r[f] for f in rr.FIELDS))(rr.resolve(i["index"], i["prob"])))


def _propagate_inputs(s):
    digits, conf = cr.frames()
    k = cr.PER_KIND
    rows = [0, k] if s == 1 else [1, 3 * k]                     # a consistent frame and a misread one; a consistent one and a contradiction
    d = digits[rows].copy()
    if s == 1:
        d[0] = np.array(cr.SELFTEST, U8).reshape(81)
    return {"digits": d, "conf": conf[rows].copy()}


case("propagate_constraints", _propagate_inputs, _dict_call("propagate_constraints", cr.FIELDS, "digits", "conf"),
     lambda i: (lambda r: tuple(r[f] for f in cr.FIELDS))(cr.propagate(i["digits"], i["conf"])))


def _solve_want(i):
    per = [sr.solve(g, 4096) for g in i["digits"]]
    return (np.stack([p[1] for p in per]).astype(U8), np.array([p[0] for p in per], np.int8), np.array([p[2] for p in per], I32))


case("solve_sudoku", lambda s: {"digits": sr.sparse_set()[4 * (s - 1):4 * (s - 1) + 2].copy()},
     _dict_call("solve_sudoku", ("solution", "result", "nodes"), "digits", max_nodes=4096), _solve_want)


# ---- K15, K16 -------------------------------------------------------------------------------------------------------------------------
MOTION = (3, 96, 160)


def _motion_inputs(s, n=MOTION[0]):
    base = _smooth(s, (n,) + MOTION[1:], tag=9)[..., None].repeat(3, -1)
    base[1, 20:60, 30:90] //= 3                                 # something moves between the frames
    base[2, 40:80, 60:130] = 255 - base[2, 40:80, 60:130]
    for f in range(3, n):
        base[f, 10 * f:10 * f + 30, 20:100 + 10 * s] //= 2
    prev = np.ascontiguousarray(stabilizer_ref.small_frame(_smooth(s, (1, 96, 160), tag=11)[0], (160, 120)), U8)
    return {"frames": np.ascontiguousarray(base), "prev_small": prev}


_motion_call = lambda c, d: c.motion_update(d["frames"], d["prev_small"], 30.0, (160, 120))
_motion_want = lambda i: (lambda small, counts: (small, counts.astype(I32)))(*stabilizer_ref.motion_counts(i["frames"], i["prev_small"], 30.0, (160, 120)))
case("motion_update", _motion_inputs, _motion_call, _motion_want)
# five frames: the per-frame counts are 20 bytes, past the 16 from which a captured hipMemsetAsync was not replayed
case("motion_update_n5", lambda s: _motion_inputs(s, 5), _motion_call, _motion_want)


def _overlay_inputs(s):
    rs = np.random.RandomState(300 + s)
    H, W = LARGE[1:]
    return {"frames": _noise(s, LARGE + (3,), tag=4), "m": np.stack([warp_ref.homography(q, 450) for q in _quads(s, 2, H, W)]),
            "digits": rs.randint(0, 10, (2, 81)).astype(U8), "classes": rs.randint(0, 3, (2, 81)).astype(U8)}


case("render_overlay", _overlay_inputs, lambda c, d: (c.render_overlay(d["frames"], d["m"], d["digits"], d["classes"]),),
     lambda i: (np.stack([overlay_ref.render(i["frames"][f], i["m"][f], i["digits"][f], i["classes"][f], atlas=overlay_ref.font_atlas()) for f in range(2)]),))


# ---- JPEG: K17 forward, K5 / K20 reconstruct, the wrappers ---------------------------------------------------------------------------
JH, JW, JQ = 24, 40, 90


def _jpeg_frames(s, gray=False):
    img = jer.content("photo", JH, JW, gray=gray)
    img = np.roll(img, 5 * s, axis=1) if s == 2 else img
    return {"frames": np.ascontiguousarray(img)[None]}


def _sparse_norm(got, i):
    masks, offsets, values, counts = got
    return masks.view(np.uint64)[0], offsets.view(np.uint32)[0], values[0, :counts[0]], counts


def _sparse_want(i):
    masks, offsets, values = jer.sparse(jer.forward(i["frames"][0], JQ, "420")[1])
    return masks, offsets, values, np.array([len(values)], I32)


case("jpeg_forward_dense", _jpeg_frames, lambda c, d: (c.jpeg_forward(d["frames"], c.jpeg_encode_plan(JW, JH, 3, JQ, "420"), dense=True),),
     lambda i: (jer.forward(i["frames"][0], JQ, "420")[1][None],))
case("jpeg_forward_sparse", _jpeg_frames, lambda c, d: c.jpeg_forward(d["frames"], c.jpeg_encode_plan(JW, JH, 3, JQ, "420")), _sparse_want, norm=_sparse_norm)


def jpeg_quant(ctx, channels):
    """the plan's quantiser steps on the device, uploaded once (outside any stream work of a case)"""
    import torch
    key = f"_stream_quant{channels}"
    if not hasattr(ctx, key):
        plan = ctx.jpeg_encode_plan(JW, JH, channels, JQ, "420")
        setattr(ctx, key, torch.from_numpy(np.array(plan.quant, np.uint16).view(np.int16).copy()).to(ctx.device))
    return getattr(ctx, key)


def _reconstruct(entry, channels, reduce=None):
    def call(c, d):
        import torch
        from sudoku_vision_amd import _native
        plan, quant = c.jpeg_encode_plan(JW, JH, channels, JQ, "420"), jpeg_quant(c, channels)
        m, of, v, _ = c.jpeg_forward(d["frames"], plan)
        r = reduce or 1
        shape = (-(-JH // r), -(-JW // r)) + ((3,) if channels == 3 else ())
        out = torch.zeros(shape, dtype=torch.uint8, device=c.device)
        args = (c._h, C.byref(plan.info), C.c_void_p(m.data_ptr()), C.c_void_p(of.data_ptr()), C.c_void_p(v.data_ptr()), C.c_void_p(quant.data_ptr()),
                C.c_void_p(out.data_ptr()), out.stride(0), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _native.check(getattr(c._lib, entry)(*args, *(() if reduce is None else (reduce,))), entry, c._lib)
        return (out,)
    return call


case("jpeg_reconstruct_sparse_bgr", _jpeg_frames, _reconstruct("sv_jpeg_reconstruct_sparse_bgr_u8", 3),
     lambda i: (o.imdecode(jer.encode(i["frames"][0], JQ, "420")),))
case("jpeg_reconstruct_sparse_scaled_bgr", _jpeg_frames, _reconstruct("sv_jpeg_reconstruct_sparse_scaled_bgr_u8", 3, 2),
     lambda i: (jpeg_reduced_ref.decode_file(jer.encode(i["frames"][0], JQ, "420"), 2),))
case("jpeg_reconstruct_sparse_gray", lambda s: _jpeg_frames(s, gray=True), _reconstruct("sv_jpeg_reconstruct_sparse_gray_u8", 1, 1),
     lambda i: (jpeg_gray_ref.decode_file(jer.encode(i["frames"][0], JQ, "gray"), 1),))
case("imencode", _jpeg_frames, lambda c, d: (c.imencode(d["frames"][0], JQ, "420"),), lambda i: (jer.pillow_encode(i["frames"][0], JQ, "420"),), kind="host")
case("imencode_batch", lambda s: {"frames": np.concatenate([_jpeg_frames(s)["frames"], _jpeg_frames(3 - s)["frames"][:, ::-1]]).copy()},
     lambda c, d: tuple(c.imencode_batch(d["frames"], 75, "422", 2, threads=2)),
     lambda i: tuple(jer.pillow_encode(f, 75, "422", 2) for f in i["frames"]), kind="host")


def _jpeg_file(width, height, seed):
    """A 4:2:0 file of random low-frequency coefficients: (height, width) is no multiple of the 16x16 MCU"""
    rs = np.random.RandomState(seed)
    mcus = -(-width // 16) * -(-height // 16)
    coef = np.zeros((6 * mcus, 64), np.int16)
    coef[:, 0] = rs.randint(-60, 61, len(coef))
    coef[:, 1:10] = rs.randint(-6, 7, (len(coef), 9))
    return jpeg_craft.write_jpeg(coef, np.full((3, 64), 8), width, height, "4:2:0")


def _jpeg_files(s):
    return _jpeg_file(40, 24, 1) if s == 1 else _jpeg_file(200, 120, 2)       # B's records outgrow A's staging set


def _out_like(c, shape):
    import torch
    return torch.zeros(shape, dtype=torch.uint8, device=c.device)


case("imdecode", _jpeg_files, lambda c, data: (c.imdecode(data),), lambda data: (o.imdecode(data),), kind="decode")
case("imdecode_reduce2", _jpeg_files, lambda c, data: (c.imdecode(data, reduce=2),), lambda data: (jpeg_reduced_ref.decode_file(data, 2),), kind="decode")
case("imdecode_gray", _jpeg_files, lambda c, data: (c.imdecode(data, gray=True),), lambda data: (jpeg_gray_ref.decode_file(data, 1),), kind="decode")
case("imdecode_dense", _jpeg_files, lambda c, data: (c.imdecode(data, dense=True),), lambda data: (o.imdecode(data),), kind="decode")
case("imdecode_out_threads", _jpeg_files,
     lambda c, data: (c.imdecode(data, threads=2, out=_out_like(c, o.imdecode(data).shape)),),
     lambda data: (o.imdecode(data),), kind="decode")
case("imdecode_batch", _jpeg_files, lambda c, data: tuple(c.imdecode_batch([data, data], threads=2)),
     lambda data: (o.imdecode(data),) * 2, kind="decode")


# ---- PNG: K18 deflate, K19 reconstruct, the wrappers ---------------------------------------------------------------------------------
PH, PW = 29, 37


def _png_frames(s):
    return {"frames": np.ascontiguousarray(np.roll(per.content("synthetic", PH, PW), 7 * (s - 1), axis=0))[None]}


def _inflate_bands(got, i):
    stream, lens, adlers, status = got
    assert not status.any()
    out, at = b"", 0
    for b, n in enumerate(lens.view(np.uint32)[0]):
        piece = zlib.decompressobj(-15).decompress(stream[0, at:at + int(n)].tobytes())
        assert int(adlers.view(np.uint32)[0, b]) == zlib.adler32(piece)
        out, at = out + piece, at + int(n)
    return (out,)


case("png_deflate", _png_frames, lambda c, d: c.png_deflate(d["frames"], c.png_encode_plan(PW, PH, 3, "paeth", "rle", 8)),
     lambda i: (per.filtered(i["frames"][0], "paeth"),), norm=_inflate_bands)
case("imencode_png", _png_frames, lambda c, d: (c.imencode_png(d["frames"][0]),), lambda i: (per.filtered(i["frames"][0], "sub"),), kind="host",
     norm=lambda got, i: (per.check_file(got[0], i["frames"][0]),))
case("imencode_png_batch", lambda s: {"frames": np.concatenate([_png_frames(s)["frames"], _png_frames(3 - s)["frames"][:, :, ::-1]]).copy()},
     lambda c, d: tuple(c.imencode_png_batch(d["frames"], "adaptive", threads=2, band_rows=8)),
     lambda i: tuple(per.filtered(f, "adaptive") for f in i["frames"]), kind="host",
     norm=lambda got, i: tuple(per.check_file(g, f) for g, f in zip(got, i["frames"])))


def _png_file(s, H=PH, W=PW, color_type=2):
    """8-bit files whose rows use all five filters, so that the segment kernel has jobs; colour type 3 with a full palette"""
    samples = png_craft.random_samples(H, W, color_type, 8, seed=s)
    palette = png_craft.random_palette(256, s) if color_type == 3 else None
    return png_craft.make_png(samples, color_type, 8, filters=[(r + s) % 5 for r in range(H)], palette=palette)


def _png_records(s, color_type):
    from sudoku_vision_amd import host
    data = _png_file(s, color_type=color_type)
    info, filtered, row_filter = host.png_inflate(data)
    d = {"_file": data, "filtered": filtered[None].copy(), "row_filter": row_filter[None].copy()}
    if color_type == 3:
        pal = np.zeros((1, 1024), U8)
        pal[0, :768] = np.frombuffer(bytes(info.palette), U8)
        pal[0, 768:772] = np.frombuffer(np.uint32(info.palette_entries).tobytes(), U8)
        d["palette"] = pal
    return d


def _png_reconstruct(c, d):
    from sudoku_vision_amd import host
    return c.png_reconstruct(host.png_parse(d["_file"]), d["filtered"], d["row_filter"], d.get("palette"))      # A's and B's geometry are one


case("png_reconstruct_rgb", lambda s: _png_records(s, 2), _png_reconstruct, lambda i: (png_decode_ref.decode(i["_file"])[None], np.zeros(1, I32)))
case("png_reconstruct_palette", lambda s: _png_records(s, 3), _png_reconstruct, lambda i: (png_decode_ref.decode(i["_file"])[None], np.zeros(1, I32)))
case("imdecode_png", lambda s: _png_file(s) if s == 1 else _png_file(s, 120, 200), lambda c, data: (c.imdecode_png(data),),
     lambda data: (png_decode_ref.decode(data),), kind="decode")
case("imdecode_png_palette", lambda s: _png_file(s, color_type=3) if s == 1 else _png_file(s, 120, 200, 3), lambda c, data: (c.imdecode_png(data),),
     lambda data: (png_decode_ref.decode(data),), kind="decode")
case("imdecode_png_batch", lambda s: _png_file(s) if s == 1 else _png_file(s, 120, 200), lambda c, data: (c.imdecode_png_batch([data, data], threads=2),),
     lambda data: (np.stack([png_decode_ref.decode(data)] * 2),), kind="decode")


def _pinned_call(c, d):
    import torch
    return (c.copy_to_pinned(d["src"], torch.zeros(d["src"].shape, dtype=torch.uint8).pin_memory()),)


case("copy_to_pinned", lambda s: {"src": _noise(s, (3, 1000))}, _pinned_call, lambda i: (i["src"],), kind="host")

PURE = [c.name for c in CASES if c.kind == "pure"]
HOST = [c.name for c in CASES if c.kind != "pure"]
CONTROLS = ("count_nonzero", "clahe", "imencode")


# ---- what the wrappers check of an input: restated for the host (tests/test_stream_cases_ref.py) -----------------------------------
_DTYPES = {"frames": U8, "gray": U8, "img": U8, "grid": U8, "binary": U8, "background": U8, "local_mean": U8, "cells": U8, "src": U8, "bits": I32,
           "minv": F64, "m": F64, "M": F64, "x": F32, "logits": F32, "index": U8, "prob": F32, "digits": U8, "conf": F32, "classes": U8,
           "prev_small": U8, "filtered": U8, "row_filter": U8, "palette": U8}


def check_input(inp):
    """The argument checks of runtime.py that look at more than the device: dtype, contiguity, and the value ranges that drive addressing."""
    if isinstance(inp, bytes):
        assert len(inp) > 0
        return
    for key, a in inp.items():
        if key.startswith("_"):
            continue
        assert isinstance(a, np.ndarray) and a.dtype == _DTYPES[key] and a.flags.c_contiguous and a.size, key
        if key in ("minv", "m"):
            assert a.shape[1:] == (3, 3) and np.isfinite(a).all() and (np.abs(np.linalg.det(a)) > 1e-12).all(), key
        if key == "digits":
            assert a.shape[1:] == (81,) and a.max() <= 9, key
        if key == "index":
            assert a.shape[1] == 81 and a.max() <= 9, key
        if key == "classes":
            assert a.max() <= 2, key
        if key == "row_filter":
            assert a.max() <= 4, key
        if key == "bits":
            assert a.shape[2] * 32 == LARGE[2], key
        if key in ("x", "logits", "prob", "conf"):
            assert np.isfinite(a).all(), key
