"""CPU: the program builder of the ml/augment_data.py drop-in against the reference's own draws (tests/golden/augment_goldens.npz,
written by tests/golden/make_augment_goldens.py), tests/augment_ref.py against the golden images, and the host entries of K22
(the program check, the matrix and tap helpers, the random words) against augment_ref."""
import ctypes as C
import math
import os
import random
import sys

import numpy as np
import pytest

import augment_ref as ar
import warp_ref

HERE = os.path.dirname(os.path.abspath(__file__))
PRESETS = ("light", "medium", "heavy")
# the Gaussian-noise cases of tests/test_gpu_augment.py: (seed, salt, H, W, sigma).  Chosen here so that no value before the
# truncation lies within 1e-9 of an integer (test_noise_cases_are_far_from_integers): the GPU test can then demand equality although
# the device's ln and cos may differ from NumPy's by a few ulp (~1e-13 at these magnitudes).
NOISE_CASES = ((5, 1234, 28, 28, 0.03 * 255), (6, 77, 13, 17, 0.05 * 255), (7, 9, 64, 64, 25.0))
NOISE_N_OUT = 3


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    import sudoku_vision_amd as sva
    if not os.path.exists(sva._native.LIB_PATH):
        g.build()
    return sva._native.lib()


@pytest.fixture(scope="module")
def aug(lib):
    import sudoku_vision_amd as sva
    ml = os.path.join(os.path.dirname(sva.__file__), "ml")
    sys.path.insert(0, ml)
    try:
        sys.modules.pop("augment_data", None)
        import augment_data
    finally:
        sys.path.remove(ml)
    return augment_data


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "augment_goldens.npz"))


def chains_of(golden):
    for c, (seed, p, k, n_aug) in enumerate(golden["chains"]):
        yield c, int(seed), PRESETS[int(p)], golden[f"image_{int(k)}"], int(n_aug)


def draw_like_the_reference(aug, seed, preset, shape, n_aug):
    """The drop-in's records for one augment_image call, identity draws kept as None."""
    random.seed(seed)
    np.random.seed(seed)
    pipeline = aug.create_augmentation_pipeline(preset)
    selected = random.sample(pipeline, min(n_aug, len(pipeline)))
    return [(a.name, a.draw(*shape)) for a in selected]


def test_step_dtype_matches_the_header(lib):
    import sudoku_vision_amd as sva
    nv = sva._native
    assert nv.AUG_STEP_DTYPE == ar.STEP_DTYPE and nv.AUG_STEP_DTYPE.itemsize == 96
    assert (nv.AUG_MAX_STEPS, nv.AUG_MAX_SIDE, nv.AUG_MAX_RADIUS) == (ar.MAX_STEPS, ar.MAX_SIDE, ar.MAX_RADIUS)
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sudoku_vision_hip.h")).read()
    for name, value in (("SV_AUG_MAX_STEPS", 10), ("SV_AUG_MAX_SIDE", 64), ("SV_AUG_MAX_RADIUS", 16)):
        assert f"#define {name} {value}" in hdr
    ops = "SV_AUG_NONE = 0, SV_AUG_AFFINE = 1, SV_AUG_PERSPECTIVE = 2, SV_AUG_BRIGHTNESS = 3, SV_AUG_CONTRAST = 4, SV_AUG_BLUR = 5"
    assert ops in hdr and "SV_AUG_SCALE = 6, SV_AUG_FILL_RECT = 7, SV_AUG_ELASTIC = 8, SV_AUG_NOISE_GAUSS = 9, SV_AUG_NOISE_SP = 10" in hdr
    assert [nv.AUG_AFFINE, nv.AUG_SCALE, nv.AUG_NOISE_SP] == [ar.AFFINE, ar.SCALE, ar.NOISE_SP]


def test_builder_records_equal_the_reference_calls(aug, golden):
    """Same operations in the same order, and every parameter the reference hands to cv2 or draws, bit for bit."""
    seen = set()
    for c, seed, preset, image, n_aug in chains_of(golden):
        got = draw_like_the_reference(aug, seed, preset, image.shape, n_aug)
        names, params, ints = golden[f"c{c}_names"], golden[f"c{c}_params"], golden[f"c{c}_ints"]
        assert [n for n, _ in got] == list(names), (c, seed, preset)
        H, W = image.shape
        for j, (name, s) in enumerate(got):
            seen.add(name)
            p, i = params[j], ints[j]
            if name in ("rotate", "translate"):
                assert s["op"] == ar.AFFINE and s["d"][:6].tobytes() == p[:6].tobytes(), (c, j, name)
            elif name == "perspective_warp":
                assert s["op"] == ar.PERSPECTIVE and s["d"].tobytes() == p.tobytes(), (c, j)
            elif name == "adjust_brightness":
                assert s["op"] == ar.BRIGHTNESS and s["d"][0] == p[0] * 255
            elif name == "adjust_contrast":
                assert s["op"] == ar.CONTRAST and s["d"][0] == p[0]
            elif name == "gaussian_blur":
                assert s["op"] == ar.BLUR and s["i"][0] == i[0]
            elif name == "add_noise":
                assert s["op"] == ar.NOISE_GAUSS and s["d"][0] == p[0] * 255
            elif name == "elastic_transform":
                r, taps = ar.elastic_taps(p[1])
                assert s["op"] == ar.ELASTIC and s["i"][0] == r and i[0] == 1
                assert s["f"][0] == np.float32(p[0]) and s["f"][1:2 + r].tobytes() == taps.tobytes()
            elif name == "scale":
                assert s["op"] == ar.SCALE and tuple(s["i"][:2]) == tuple(i[:2])
                assert s["i"][2] == (1 if (i[0] > W or i[1] > H) else 0) or (i[0] == W and i[1] == H)
            else:
                assert name == "random_erasing" and (s is None or s["op"] == ar.FILL_RECT)
    assert seen == {"rotate", "translate", "perspective_warp", "adjust_brightness", "adjust_contrast", "gaussian_blur", "add_noise", "elastic_transform",
                    "scale", "random_erasing"}


def test_reference_arithmetic_equals_augment_ref(aug, golden):
    """Every deterministic function's recorded output (the reference's own numpy arithmetic, and the restated cv2 calls it made) from
    its recorded input and the drop-in's step record; whole light and medium chains give the golden image."""
    whole = 0
    for c, seed, preset, image, n_aug in chains_of(golden):
        got = draw_like_the_reference(aug, seed, preset, image.shape, n_aug)
        gin, gout = golden[f"c{c}_in"], golden[f"c{c}_out"]
        for j, (name, s) in enumerate(got):
            if name in ("add_noise", "elastic_transform"):
                continue
            out = gin[j].copy() if s is None else ar.apply_step(gin[j], s)
            assert (out == gout[j]).all(), (c, j, name)
        if preset != "heavy":
            steps, n_steps = ar.program([[s for _, s in got if s is not None]])
            assert (ar.run_program(image[None], steps, n_steps, [0])[0] == gout[-1]).all()
            whole += 1
    assert whole == 16


def test_build_program_is_the_loop(aug):
    random.seed(3)
    np.random.seed(3)
    steps, n_steps, src_index = aug.build_program(3, 28, 28, 4, aug.create_augmentation_pipeline("heavy"), 3)
    random.seed(3)
    np.random.seed(3)
    pipeline = aug.create_augmentation_pipeline("heavy")
    chains = [aug.draw_chain(28, 28, pipeline, 3) for _ in range(12)]
    assert list(src_index) == [0] * 4 + [1] * 4 + [2] * 4 and list(n_steps) == [len(c) for c in chains]
    for k, c in enumerate(chains):
        assert steps[k, :len(c)].tobytes() == b"".join(s.tobytes() for s in c)
    with pytest.raises(ValueError, match="4..64"):
        aug.build_program(1, 3, 28, 1, pipeline)
    with pytest.raises(ValueError, match="4..64"):
        aug.build_program(1, 28, 65, 1, pipeline)


def test_host_helpers_equal_augment_ref(lib):
    m = (C.c_double * 6)()
    for cx, cy, angle in ((14, 14, 7.3), (8, 6, -15.0), (32, 32, 0.0), (14, 14, 1e-3)):
        assert lib.sv_augment_rotation_matrix(float(cx), float(cy), angle, 1.0, m) == 0
        assert np.array(m).tobytes() == ar.rotation_matrix((cx, cy), angle).tobytes()
    rs = np.random.RandomState(0)
    m9 = (C.c_double * 9)()
    for h, w in ((28, 28), (13, 17), (64, 64)):
        src = np.float32([[0, 0], [w, 0], [w, h], [0, h]])
        dst = (src + rs.uniform(-0.1, 0.1, (4, 2)).astype(np.float32) * np.float32([w, h])).astype(np.float32)
        assert lib.sv_augment_perspective_matrix(src.ctypes.data, dst.ctypes.data, m9) == 0
        assert np.array(m9).tobytes() == ar.perspective_matrix(src, dst).tobytes()
    assert lib.sv_augment_perspective_matrix(np.zeros(8, np.float32).ctypes.data, np.zeros(8, np.float32).ctypes.data, m9) == -5
    taps, radius = (C.c_float * 17)(), C.c_int()
    for sigma in (3.0, 4.0, 1.0, 0.5, 2.7):
        assert lib.sv_augment_elastic_taps(sigma, taps, 17, C.byref(radius)) == 0
        r, want = ar.elastic_taps(sigma)
        assert radius.value == r == (int(round(8 * sigma + 1)) | 1) // 2 and np.array(taps[:r + 1], np.float32).tobytes() == want.tobytes()
        full = np.concatenate([want[:0:-1], want]).astype(np.float64)
        assert abs(full.sum() - 1) < 1e-6
    assert lib.sv_augment_elastic_taps(5.0, taps, 17, C.byref(radius)) == -6 and radius.value == 20
    assert lib.sv_augment_elastic_taps(0.0, taps, 17, C.byref(radius)) == -1
    assert lib.sv_augment_elastic_taps(float("nan"), taps, 17, C.byref(radius)) == -1


def test_host_field_equals_augment_ref(lib):
    # Philox4x32-10's published known-answer vectors (Random123 kat_vectors)
    assert [int(w) for w in ar.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(w) for w in ar.philox4x32_10(0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    for seed, index, slot, salt, H, W in ((0, 0, 0, 0, 4, 4), (2 ** 64 - 1, 2 ** 56 - 1, 9, 2 ** 32 - 1, 13, 17), (12345678901234, 2 ** 33 + 5, 3, 77, 64, 64)):
        words = np.empty((H, W, 4), np.uint32)
        assert lib.sv_augment_field_host(seed, index, slot, salt, H, W, words.ctypes.data) == 0
        assert (words == ar.field_words(seed, index, slot, salt, H, W)).all()
    assert lib.sv_augment_field_host(0, 2 ** 56, 0, 0, 4, 4, words.ctypes.data) == -1
    u = ar.uniform_pm1(np.array([0, 0xff, 0x100, 0xffffffff], np.uint32))
    assert u.dtype == np.float32 and list(u) == [-1.0, -1.0, -1.0 + 2.0 ** -23, 1.0 - 2.0 ** -23]


def test_perspective_coords_equal_warp_ref_on_a_square():
    src = np.float32([[0, 0], [28, 0], [28, 28], [0, 28]])
    dst = src + np.float32([[1.5, -2], [-2.25, 1], [0.5, 2.5], [2, -1]])
    minv = ar.invert3(ar.perspective_matrix(src, dst))
    X, Y = ar.perspective_coords(minv, 28, 28)
    _, _, _, _, Xw, Yw = warp_ref.coords(minv, 28)
    assert (X == Xw).all() and (Y == Yw).all()
    # inside the image a replicated border is the constant-border sample of warp_ref
    img = ar.sample_image(28, 28)
    inside = (X >> 5 >= 0) & (X >> 5 < 27) & (Y >> 5 >= 0) & (Y >> 5 < 27)
    assert inside.sum() > 300
    assert (ar.warp_perspective(img, ar.perspective_matrix(src, dst))[inside] == warp_ref.warp(img, minv, 28)[inside]).all()


def _check(lib, chains, n_src=1, H=28, W=28, src_index=None, n_steps=None):
    steps, ns = ar.program(chains)
    ns = ns if n_steps is None else np.array(n_steps, np.int32)
    si = np.zeros(len(chains), np.int32) if src_index is None else np.array(src_index, np.int32)
    rc = lib.sv_augment_check_program(steps.ctypes.data, ns.ctypes.data, si.ctypes.data, len(chains), n_src, H, W)
    return rc, lib.sv_last_error().decode()


def test_check_program(lib, aug):
    S = ar.step
    r, taps = ar.elastic_taps(3.0)
    good = [S(ar.AFFINE, d=[1, 0, 2, 0, 1, -1]), S(ar.PERSPECTIVE, d=[1, 0, 0, 0, 1, 0, 0, 0, 1]), S(ar.BRIGHTNESS, d=[-300]), S(ar.CONTRAST, d=[1.2]),
            S(ar.BLUR, i=[5]), S(ar.SCALE, i=[30, 30, 1]), S(ar.SCALE, i=[25, 26, 0]), S(ar.FILL_RECT, i=[27, 27, 1, 1, 255]),
            S(ar.ELASTIC, i=[r, 0, 0, 0, 5], f=[8.0] + list(taps)), S(ar.NOISE_GAUSS, d=[7.65])]
    assert _check(lib, [good, [], [S(ar.NONE), S(ar.NOISE_SP, d=[0.025])]])[0] == 0
    bad = {
        "unknown op 11": S(11), "unknown op -1": S(-1),
        "affine matrix is not finite": S(ar.AFFINE, d=[1, 0, np.inf, 0, 1, 0]),
        "perspective matrix is not finite": S(ar.PERSPECTIVE, d=[1, 0, 0, 0, 1, 0, 0, 0, np.nan]),
        "parameter is not finite": S(ar.CONTRAST, d=[np.nan]),
        "blur kernel 7": S(ar.BLUR, i=[7]), "blur kernel 2": S(ar.BLUR, i=[2]),
        "scale to 27 x 29": S(ar.SCALE, i=[29, 27, 1]), "scale to 29 x 28": S(ar.SCALE, i=[28, 29, 0]), "scale to 57 x 28": S(ar.SCALE, i=[28, 57, 1]),
        "scale to 0 x 5": S(ar.SCALE, i=[5, 0, 0]),
        "rectangle x 27 y 0 w 2": S(ar.FILL_RECT, i=[27, 0, 2, 1, 0]), "rectangle x -1": S(ar.FILL_RECT, i=[-1, 0, 1, 1, 0]),
        "value 256": S(ar.FILL_RECT, i=[0, 0, 1, 1, 256]), "rectangle x 2147483647": S(ar.FILL_RECT, i=[2 ** 31 - 1, 0, 2 ** 31 - 1, 1, 0]),
        "elastic radius 17": S(ar.ELASTIC, i=[17], f=[8.0]), "elastic radius -1": S(ar.ELASTIC, i=[-1, 0, 0, 0, 0], f=[8.0]),
        "tap 3 is not finite": S(ar.ELASTIC, i=[4, 0, 0, 0, 0], f=[8.0, 0.2, 0.2, np.nan, 0.1, 0.1]),
    }
    for text, s in bad.items():
        rc, msg = _check(lib, [[good[0]], [good[3], s]])
        assert rc == -1 and "output 1 step 1" in msg and text in msg, (text, msg)
    # the sigma = 3 elastic needs min(H, W) >= 13: REFLECT_101 reflects once
    el = good[8]
    assert _check(lib, [[el]], H=13, W=17)[0] == 0
    rc, msg = _check(lib, [[el]], H=12, W=17)
    assert rc == -1 and "output 0 step 0: elastic radius 12" in msg
    assert _check(lib, [[]], src_index=[1])[0] == -1 and "source index 1" in lib.sv_last_error().decode()
    assert _check(lib, [[]], src_index=[-1])[0] == -1
    assert _check(lib, [[]], n_steps=[11])[0] == -1 and "11 steps" in lib.sv_last_error().decode()
    assert _check(lib, [[]], n_steps=[-1])[0] == -1
    assert _check(lib, [[]], H=3)[0] == -1 and _check(lib, [[]], W=65)[0] == -1
    # a slot beyond n_steps is not looked at
    assert _check(lib, [[good[0], S(99)]], n_steps=[1])[0] == 0
    import sudoku_vision_amd as sva
    steps, ns = ar.program([[S(ar.BLUR, i=[4])]])
    with pytest.raises(sva._native.NativeError, match="SV_ERR_BAD_ARG.*output 0 step 0"):
        sva.Context.augment_check_program(steps, ns, [0], 1, 28, 28)


def noise_fields():
    for seed, salt, H, W, sigma in NOISE_CASES:
        imgs = ar.sample_images(NOISE_N_OUT, H, W, seed)
        for o in range(NOISE_N_OUT):
            yield imgs[o], ar.field_words(seed, 1000 + o, 0, salt, H, W), sigma


def test_noise_cases_are_far_from_integers():
    for img, words, sigma in noise_fields():
        v = ar.noise_gauss_values(img, words, sigma)
        assert np.abs(v - np.rint(v)).min() > 1e-9


def test_noise_statistics_of_the_reference():
    """|mean| < 5 / sqrt(N), |std - 1| < 5 / sqrt(2N) for the normals the GPU test draws; salt and pepper rates within 5 sigma."""
    z = np.concatenate([ar.normal(w[..., 0], w[..., 1]).ravel() for _, w, _ in noise_fields()])
    N = z.size
    assert N == NOISE_N_OUT * (28 * 28 + 13 * 17 + 64 * 64)
    assert abs(z.mean()) < 5 / math.sqrt(N) and abs(z.std() - 1) < 5 / math.sqrt(2 * N)
    u = np.concatenate([ar.uniform01(w[..., :2]).ravel() for _, w, _ in noise_fields()])
    p = 0.1
    assert abs((u < p).mean() - p) < 5 * math.sqrt(p * (1 - p) / u.size)
    f = np.concatenate([ar.uniform_pm1(w[..., :2]).ravel() for _, w, _ in noise_fields()])
    assert abs(f.mean()) < 5 / math.sqrt(3 * f.size) and f.min() >= -1 and f.max() < 1
