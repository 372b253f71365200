"""CPU: the job builder of the ml/generate_synthetic_v2.py drop-in against the reference's own draws and images
(tests/golden/synth_cells_goldens.npz, written by tests/golden/make_synth_cells_goldens.py), tests/synth_cells_ref.py against the golden
images, the host entries of K23 (the job check, the tap helper) against synth_cells_ref, and the vetting of the cases the GPU tests use."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

import augment_ref as ar
import synth_cells_ref as sr

HERE = os.path.dirname(os.path.abspath(__file__))
S = ar.step
# the Gaussian-field cases of tests/test_gpu_synth_cells.py: (seed, salt, size, base, sigma, kind).  Chosen here so that no value before the
# truncation lies within 1e-9 of an integer (test_field_cases_are_far_from_integers): the GPU test can then demand equality although the
# device's ln and cos may differ from NumPy's by a few ulp.
FIELD_CASES = ((5, 1234, 28, 245, 3.5, sr.TEXTURED), (6, 77, 12, 250, 7.9, sr.NOISY), (7, 9, 64, 240, 2.1, sr.TEXTURED), (8, 4321, 4, 255, 5.0, sr.NOISY))
FIELD_N_OUT = 3
FIELD_BASE = 1000
# the seeded cell set of the GPU drop-in tests: generate_batch(BATCH_LABELS) under seed_all(BATCH_SEED)
BATCH_SEED, BATCH_LABELS, BATCH_FIELD_SEED = 3, [0] * 14 + list(range(1, 10)) * 3, 11


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    import sudoku_vision_amd as sva
    if not os.path.exists(sva._native.LIB_PATH):
        g.build()
    return sva._native.lib()


@pytest.fixture(scope="module")
def gen(lib):
    return load_dropin()


def load_dropin():
    import sudoku_vision_amd as sva
    ml = os.path.join(os.path.dirname(sva.__file__), "ml")
    sys.path.insert(0, ml)
    try:
        sys.modules.pop("generate_synthetic_v2", None)
        import generate_synthetic_v2
    finally:
        sys.path.remove(ml)
    return generate_synthetic_v2


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "synth_cells_goldens.npz"))


class GoldenFont:
    """The glyph source of one golden cell: what the maker's Pillow font gave."""

    def __init__(self, g, c):
        self.mask, self.meta = g[f"c{c}_mask"], [int(v) for v in g[f"c{c}_glyph"]]

    def glyph(self, digit):
        return self.mask, (self.meta[0], self.meta[1]), tuple(self.meta[2:])


class RingFont:
    """A glyph source that needs no font: a ring mask per digit, the size of a size-24 glyph."""

    def glyph(self, digit):
        return sr.sample_mask(18 + digit % 3, 11 + digit % 5, digit), (1, 5 + digit % 2), (1, 5, 12 + digit % 5, 23)


def seed_all(s):
    random.seed(s)
    np.random.seed(s)


def golden_jobs(gen, g):
    for c, (seed, label, size, font_size, whole, bg_normals) in enumerate(g["cells"]):
        seed_all(int(seed))
        fonts = [("golden", GoldenFont(g, c) if label else None)]
        cells, steps, n_steps, atlas = gen.build_cells([int(label)], fonts, int(size))
        yield c, int(label), int(size), bool(whole), int(bg_normals), cells, steps, n_steps, atlas


def test_dtypes_match_the_header(lib):
    import sudoku_vision_amd as sva
    nv = sva._native
    assert nv.SYN_CELL_DTYPE == sr.CELL_DTYPE and nv.SYN_CELL_DTYPE.itemsize == 96
    assert (nv.SYN_GLYPH_SIDE, nv.SYN_BG_SLOT) == (sr.GLYPH_SIDE, sr.BG_SLOT)
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sudoku_vision_hip.h")).read()
    assert "#define SV_SYN_GLYPH_SIDE 32" in hdr and "#define SV_SYN_BG_SLOT 255" in hdr
    assert "SV_SYN_AFFINE_CONST = 32, SV_SYN_PERSPECTIVE_CONST = 33, SV_SYN_SCALE_PAD = 34, SV_SYN_GAUSS_BLUR = 35, SV_SYN_ERODE = 36, SV_SYN_DILATE = 37" in hdr
    assert "SV_SYN_BG_PLAIN = 0, SV_SYN_BG_TEXTURED = 1, SV_SYN_BG_GRADIENT = 2, SV_SYN_BG_NOISY = 3, SV_SYN_BG_KEEP = 4" in hdr
    assert [nv.SYN_AFFINE_CONST, nv.SYN_DILATE, nv.SYN_BG_KEEP] == [sr.AFFINE_CONST, sr.DILATE, sr.KEEP]


def test_build_cells_consumes_the_recorded_draws(gen, golden):
    """After the drop-in has drawn a golden cell under its seed, Python's generator stands where the reference left it."""
    for c, *_ in golden_jobs(gen, golden):
        assert random.random() == float(golden[f"c{c}_next"]), c


def test_records_equal_the_reference_calls(gen, golden):
    """Every parameter the reference hands to cv2 and to np.random, bit for bit, in its order."""
    seen = set()
    for c, label, size, whole, bg_normals, cells, steps, n_steps, atlas in golden_jobs(gen, golden):
        names, params, normals = list(golden[f"c{c}_cv_names"]), golden[f"c{c}_cv_params"], [float(v) for v in golden[f"c{c}_normal"][:, 0]]
        cell = cells[0]
        if int(cell["bg_kind"]) in (sr.TEXTURED, sr.NOISY):
            assert bg_normals == 1 and cell["bg_d"][0] == normals.pop(0)
        else:
            assert bg_normals == 0
        k = 0
        for s in steps[0, :n_steps[0]]:
            op = int(s["op"])
            seen.add(op)
            if op == sr.AFFINE_CONST:
                assert names[k] == "warpAffine" and s["d"][:6].tobytes() == params[k][:6].tobytes() and s["i"][0] == params[k][6] == 255
            elif op == sr.PERSPECTIVE_CONST:
                assert names[k] == "warpPerspective" and s["d"].tobytes() == params[k][:9].tobytes() and s["i"][0] == params[k][9] == 255
            elif op == sr.SCALE_PAD:
                assert names[k] == "resize" and tuple(s["i"][:2]) == tuple(params[k][:2])
                if s["i"][2] == 0:
                    k += 1
                    pad = (size - s["i"][0]) // 2
                    assert names[k] == "copyMakeBorder" and list(params[k][:5]) == [pad, size - s["i"][0] - pad, pad, size - s["i"][0] - pad, 255] and s["i"][3] == 255
                else:
                    assert s["i"][0] > size
            elif op == sr.GAUSS_BLUR:
                assert names[k] == "GaussianBlur" and s["i"][0] == params[k][0] and list(s["i"][1:4]) == sr.gaussian_taps_q8(int(params[k][0]), params[k][1])
            elif op in (sr.ERODE, sr.DILATE):
                assert names[k] == ("erode" if op == sr.ERODE else "dilate")
            elif op == ar.NOISE_GAUSS:
                assert s["d"][0] == normals.pop(0)
                continue
            else:
                assert op in (ar.BRIGHTNESS, ar.CONTRAST)
                continue
            k += 1
        assert k == len(names) and not normals, c
    assert seen == {sr.AFFINE_CONST, sr.PERSPECTIVE_CONST, sr.SCALE_PAD, sr.GAUSS_BLUR, sr.ERODE, sr.DILATE, ar.BRIGHTNESS, ar.CONTRAST, ar.NOISE_GAUSS}


def test_reference_arithmetic_equals_the_restatement(gen, golden):
    """The reference's own numpy and Pillow arithmetic, from the drop-in's records: base images without a Gaussian field, artefacts on the
    recorded input, every step up to the first noise step, and whole cells where no field was drawn."""
    bases = wholes = arts = 0
    kinds = set()
    for c, label, size, whole, bg_normals, cells, steps, n_steps, atlas in golden_jobs(gen, golden):
        cell = cells[0]
        if f"c{c}_art_in" in golden:
            assert (sr.artefacts(golden[f"c{c}_art_in"], int(cell["art_edges"]), int(cell["art_width"]), int(cell["art_dark"])) == golden[f"c{c}_art_out"]).all(), c
            arts += 1
        if bg_normals == 0:
            kinds.add((int(cell["bg_kind"]), int(cell["grad_dir"]) if cell["bg_kind"] == sr.GRADIENT else -1))
            assert (sr.background(cell, size) == golden[f"c{c}_bg"]).all(), c
            assert (sr.base_image(cell, size, atlas) == golden[f"c{c}_base"]).all(), c
            bases += 1
        else:                                                  # the field is NumPy's: restate what the reference did to its recorded background
            kept = cell.copy()
            kept["bg_kind"] = sr.KEEP
            prev = golden[f"c{c}_bg"].copy()
            if int(cell["grain_stride"]):                     # the recorded background has the grain in it already
                kept["grain_stride"] = 0
            assert (sr.base_image(kept, size, atlas, prev=prev) == golden[f"c{c}_base"]).all(), c
        img = golden[f"c{c}_base"]
        for slot, s in enumerate(steps[0, :n_steps[0]]):
            if int(s["op"]) == ar.NOISE_GAUSS:
                break
            img = sr.apply_step(img, s)
        else:
            assert (img == golden[f"c{c}_out"]).all(), c
            wholes += 1
    assert bases >= 10 and wholes >= 3 and arts >= 2
    assert kinds >= {(sr.PLAIN, -1), (sr.GRADIENT, 0), (sr.GRADIENT, 1), (sr.GRADIENT, 2)}


def test_grain_equals_the_reference(gen, golden):
    """A textured background with grain: the drop-in's packed d rows, applied to the field the reference drew, give the reference's rows."""
    n = 0
    for c, label, size, whole, bg_normals, cells, steps, n_steps, atlas in golden_jobs(gen, golden):
        cell = cells[0]
        if int(cell["grain_stride"]):
            bg = golden[f"c{c}_bg"]
            stride, bits = int(cell["grain_stride"]), int(cell["grain_d"][0]) | int(cell["grain_d"][1]) << 32
            d = [(bits >> (2 * k)) & 3 for k in range(len(range(0, size, stride)))]
            assert all(1 <= v <= 3 for v in d)
            rows = bg[::stride].astype(int)
            other = np.delete(bg, np.arange(0, size, stride), axis=0).astype(int)
            assert rows.mean() < other.mean()                                       # the grain rows are the darker ones
            n += 1
    assert n >= 1


def test_linspace_terms_are_numpys():
    for strength, size in ((3.0, 28), (9.99, 12), (7.123456789, 64), (5.5, 4)):
        start, step, stop = sr.linspace_terms(strength, size)
        t = np.arange(size, dtype=np.float64) * step + start
        t[-1] = stop
        assert t.tobytes() == np.linspace(-strength, strength, size).tobytes()


def test_mask_paste_equals_imagedraw_text():
    """Pillow's draw.text on a white canvas = the blend of ink through getmask2's mask pasted at (x + off_x, y + off_y)."""
    PIL = pytest.importorskip("PIL")
    from PIL import Image, ImageDraw, ImageFont, features
    if not features.check("freetype2"):
        pytest.skip("Pillow without FreeType")
    n = 0
    for fs in range(16, 25):
        font = ImageFont.load_default(size=fs)
        for digit in range(1, 10):
            for ink, (x, y) in ((0, (14, 9)), (30, (-3, 20)), (17, (40, -6))):
                canvas = Image.new("L", (48, 48), color=255)
                ImageDraw.Draw(canvas).text((x, y), str(digit), font=font, fill=ink)
                mask, off = font.getmask2(str(digit), mode="L")
                m = np.array(mask, np.uint8).reshape(mask.size[1], mask.size[0])
                assert (sr.digit_layer(48, m, x + off[0], y + off[1], ink) == np.array(canvas)).all(), (fs, digit, ink)
                assert m.shape[0] <= sr.GLYPH_SIDE and m.shape[1] <= sr.GLYPH_SIDE
                n += 1
    assert n == 243


def test_taps_helper(lib):
    t = (C.c_int32 * 3)()
    for k in (3, 5):
        for sigma in (0.3, 0.5, 0.77, 1.0, 2.5, 1e-3, 1e3):
            assert lib.sv_synth_gaussian_taps_q8(k, sigma, t) == 0
            assert list(t) == sr.gaussian_taps_q8(k, sigma) and t[0] + 2 * t[1] + 2 * t[2] == 256 and min(t) >= 0 and (k == 5 or t[2] == 0)
    for k, sigma in ((4, 1.0), (7, 1.0), (3, 0.0), (3, -1.0), (5, float("nan")), (5, float("inf"))):
        assert lib.sv_synth_gaussian_taps_q8(k, sigma, t) == -1


def _check(lib, cells, chains=None, size=28, dims=((11, 18),), n_steps=None):
    cells = sr.cells_array(cells)
    steps, ns = ar.program(chains if chains is not None else [[]] * len(cells))
    ns = ns if n_steps is None else np.array(n_steps, np.int32)
    d = np.array(dims, np.int32).reshape(-1, 2)
    rc = lib.sv_synth_check_program(cells.ctypes.data, steps.ctypes.data, ns.ctypes.data, len(cells), size, d.ctypes.data if len(d) else None, len(d))
    return rc, lib.sv_last_error().decode()


def test_check_program(lib):
    cell = sr.cell
    good_cells = [cell(), cell(sr.TEXTURED, 245, 7, grain=(2, [1, 2, 3] * 5), bg_d=[3.0]), cell(sr.GRADIENT, 250, grad_dir=2, bg_d=[9.0]),
                  cell(sr.GRADIENT, 250, grad_dir=1, bg_d=sr.linspace_terms(5.0, 28)), cell(sr.NOISY, 255, -1, bg_d=[8.0]),
                  cell(art=(15, 2, 180), smudge=(23, 0, 5, 210)), cell(glyph=(0, -40, 90, 30)), cell(sr.KEEP)]
    good_steps = [S(sr.AFFINE_CONST, i=[255], d=[1, 0, 2, 0, 1, -1]), S(sr.PERSPECTIVE_CONST, i=[0], d=[1, 0, 0, 0, 1, 0, 0, 0, 1]), S(sr.SCALE_PAD, i=[1, 1, 0, 255]),
                  S(sr.SCALE_PAD, i=[34, 34, 1, 255]), S(sr.GAUSS_BLUR, i=[5, 102, 62, 15]), S(sr.GAUSS_BLUR, i=[3, 254, 1, 0]), S(sr.ERODE), S(sr.DILATE),
                  S(ar.BRIGHTNESS, d=[-15]), S(ar.NOISE_GAUSS, d=[7.65])]
    assert _check(lib, good_cells, [good_steps] + [[]] * 7)[0] == 0
    bad_cells = {
        "bg_kind: unknown kind 5": cell(5), "bg_kind: unknown kind -1": cell(-1), "bg_value: 256": cell(bg_value=256), "bg_value: -1": cell(bg_value=-1),
        "bg_d: sigma is not finite": cell(sr.NOISY, bg_d=[np.nan]), "grad_dir: unknown direction 3": cell(sr.GRADIENT, grad_dir=3),
        "bg_d: gradient term is not finite": cell(sr.GRADIENT, grad_dir=0, bg_d=[0, np.inf, 0]),
        "grain_stride: 5": cell(sr.TEXTURED, grain=(5, [1] * 32), bg_d=[1]), "grain_stride: 1": cell(sr.TEXTURED, grain=(1, [1] * 32), bg_d=[1]),
        "grain_d: row 4 has d 0": cell(sr.TEXTURED, grain=(2, [1, 1, 0] + [1] * 20), bg_d=[1]),
        "art_edges: 16": cell(art=(16, 1, 200)), "art_width: 3": cell(art=(1, 3, 200)), "art_width: 0": cell(art=(1, 0, 200)), "art_dark: 300": cell(art=(1, 1, 300)),
        "smudge: x 24 y 0 side 5": cell(smudge=(24, 0, 5, 210)), "smudge: x -1": cell(smudge=(-1, 0, 2, 210)), "darkness 256": cell(smudge=(0, 0, 2, 256)),
        "smudge: x 0 y 0 side 29": cell(smudge=(0, 0, 29, 210)), "smudge: x 2147483647": cell(smudge=(2 ** 31 - 1, 0, 2 ** 31 - 1, 0)),
        "glyph_slot: 1 outside -1..0": cell(glyph=(1, 0, 0, 0)), "glyph_slot: -2": cell(glyph=(-2, 0, 0, 0)), "glyph_ink: 256": cell(glyph=(0, 0, 0, 256)),
    }
    for text, c in bad_cells.items():
        rc, msg = _check(lib, [cell(), c])
        assert rc == -1 and "output 1 " in msg and text in msg, (text, msg)
    bad_steps = {
        "unknown op 38": S(38), "unknown op 31": S(31), "unknown op 11": S(11), "unknown op -1": S(-1),
        "affine matrix is not finite": S(sr.AFFINE_CONST, i=[255], d=[1, 0, np.inf, 0, 1, 0]), "border value 256": S(sr.AFFINE_CONST, i=[256], d=[1, 0, 0, 0, 1, 0]),
        "perspective matrix is not finite": S(sr.PERSPECTIVE_CONST, d=[1, 0, 0, 0, 1, 0, 0, 0, np.nan]), "border value -1": S(sr.PERSPECTIVE_CONST, i=[-1], d=[1, 0, 0, 0, 1, 0, 0, 0, 1]),
        "scale to 27 x 29": S(sr.SCALE_PAD, i=[29, 27, 1, 255]), "scale to 0 x 5": S(sr.SCALE_PAD, i=[5, 0, 0, 255]), "scale to 57 x 57": S(sr.SCALE_PAD, i=[57, 57, 1, 255]),
        "pad value 300": S(sr.SCALE_PAD, i=[20, 20, 0, 300]),
        "blur kernel 1": S(sr.GAUSS_BLUR, i=[1, 256, 0, 0]), "blur kernel 7": S(sr.GAUSS_BLUR, i=[7, 256, 0, 0]),
        "blur taps 100 62 15 do not sum to 256": S(sr.GAUSS_BLUR, i=[5, 100, 62, 15]), "blur taps 258 -1 0": S(sr.GAUSS_BLUR, i=[3, 258, -1, 0]),
        "blur taps 102 62 15": S(sr.GAUSS_BLUR, i=[3, 102, 62, 15]),
        "parameter is not finite": S(ar.CONTRAST, d=[np.nan]), "blur kernel 4": S(ar.BLUR, i=[4]), "elastic radius 17": S(ar.ELASTIC, i=[17], f=[8.0]),
    }
    for text, s in bad_steps.items():
        rc, msg = _check(lib, [cell(), cell()], [[good_steps[0]], [good_steps[6], s]])
        assert rc == -1 and "output 1 step 1" in msg and text in msg, (text, msg)
    rc, msg = _check(lib, [cell()], dims=((33, 10),))
    assert rc == -1 and "atlas slot 0: mask of 33 x 10" in msg
    assert _check(lib, [cell()], dims=((10, 0),))[0] == -1
    assert _check(lib, [cell()], dims=())[0] == 0 and _check(lib, [cell(glyph=(0, 0, 0, 0))], dims=())[0] == -1
    assert _check(lib, [cell()], n_steps=[11])[0] == -1 and "11 steps" in lib.sv_last_error().decode()
    assert _check(lib, [cell()], n_steps=[-1])[0] == -1
    assert _check(lib, [cell()], size=3)[0] == -1 and _check(lib, [cell()], size=65)[0] == -1
    assert _check(lib, [cell()], [[good_steps[0], S(99)]], n_steps=[1])[0] == 0           # a slot beyond n_steps is not looked at
    import sudoku_vision_amd as sva
    with pytest.raises(sva._native.NativeError, match="SV_ERR_BAD_ARG.*output 0 step 0"):
        sva.Context.synth_check_program(sr.cells_array([cell()]), ar.program([[S(40)]])[0], [1], 28, np.zeros((0, 2), np.int32))
    with pytest.raises(ValueError, match="1..32"):
        sva.Context.synth_atlas([np.zeros((33, 4), np.uint8)])


def test_k22_check_still_refuses_the_new_ops(lib):
    for op in range(sr.AFFINE_CONST, sr.DILATE + 1):
        steps, ns = ar.program([[S(op, i=[255, 3, 0, 255], d=[1, 0, 0, 0, 1, 0, 0, 0, 1])]])
        si = np.zeros(1, np.int32)
        assert lib.sv_augment_check_program(steps.ctypes.data, ns.ctypes.data, si.ctypes.data, 1, 1, 28, 28) == -1
        assert f"unknown op {op}" in lib.sv_last_error().decode()


def field_cells():
    for seed, salt, size, base, sigma, kind in FIELD_CASES:
        grain = (2, [1 + k % 3 for k in range(32)]) if kind == sr.TEXTURED else None
        for o in range(FIELD_N_OUT):
            yield seed, FIELD_BASE + o, size, sr.cell(kind, base, salt, grain=grain, bg_d=[sigma])


def test_field_cases_are_far_from_integers():
    for seed, index, size, c in field_cells():
        v = sr.background_values(c, size, seed, index)
        assert np.abs(v - np.rint(v)).min() > 1e-9
    assert sr.BG_SLOT >= ar.MAX_STEPS                          # no step can have phase A's slot


def test_batch_noise_is_far_from_integers(gen):
    """The same condition for every Gaussian field of the seeded batch the GPU drop-in tests draw, noise steps included."""
    seed_all(BATCH_SEED)
    cells, steps, n_steps, atlas = gen.build_cells(BATCH_LABELS, [("ring", RingFont())], 28)
    for o in range(len(cells)):
        if int(cells[o]["bg_kind"]) in (sr.TEXTURED, sr.NOISY):
            v = sr.background_values(cells[o], 28, BATCH_FIELD_SEED, o)
            assert np.abs(v - np.rint(v)).min() > 1e-9, o
        img = sr.base_image(cells[o], 28, atlas, BATCH_FIELD_SEED, o)
        for slot in range(n_steps[o]):
            s = steps[o, slot]
            if int(s["op"]) == ar.NOISE_GAUSS:
                v = ar.noise_gauss_values(img, ar.field_words(BATCH_FIELD_SEED, o, slot, int(s["i"][4]), 28, 28), s["d"][0])
                assert np.abs(v - np.rint(v)).min() > 1e-9, (o, slot)
            img = sr.apply_step(img, s, BATCH_FIELD_SEED, o, slot)


def test_batch_covers_every_branch(gen):
    """The seeded cell set of the GPU tests contains every background kind, gradient direction, grain on and off, each artefact edge, a
    smudge, every augmentation step and both morphology ops: a change of seed cannot silently drop a branch."""
    seed_all(BATCH_SEED)
    cells, steps, n_steps, atlas = gen.build_cells(BATCH_LABELS, [("ring", RingFont())], 28)
    assert set(cells["bg_kind"]) == {sr.PLAIN, sr.TEXTURED, sr.GRADIENT, sr.NOISY}
    assert set(cells["grad_dir"][cells["bg_kind"] == sr.GRADIENT]) == {0, 1, 2}
    textured = cells[cells["bg_kind"] == sr.TEXTURED]
    assert (textured["grain_stride"] > 0).any() and (textured["grain_stride"] == 0).any()
    for bit in (1, 2, 4, 8):
        assert (cells["art_edges"] & bit).any()
    assert (cells["smudge"][:, 2] > 0).any() and (cells["glyph_slot"] >= 0).sum() == 27
    ops = {int(steps[o, k]["op"]) for o in range(len(cells)) for k in range(n_steps[o])}
    assert ops == {sr.AFFINE_CONST, sr.SCALE_PAD, sr.GAUSS_BLUR, ar.BRIGHTNESS, ar.CONTRAST, ar.NOISE_GAUSS, sr.PERSPECTIVE_CONST, sr.ERODE, sr.DILATE}
    assert {int(s["i"][2]) for o in range(len(cells)) for s in steps[o, :n_steps[o]] if s["op"] == sr.SCALE_PAD} == {0, 1}
