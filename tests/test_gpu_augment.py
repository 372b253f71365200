"""GPU: K22 (sv_augment_u8, Context.augment) and the ml/augment_data.py drop-in, bit for bit against tests/augment_ref.py.

Shapes: 28 x 28; 13 x 17 (odd, and the smallest the sigma = 3 elastic step admits); 4 x 4 (the floor, without elastic); 64 x 64 (the
ceiling); n_out of 1, 3 and 257.  The images are gradients plus noise, never constant (a replicated and a constant border differ),
but for the one flat image the contrast step is also run on.

The Gaussian noise is compared for equality although the device's ln and cos may differ from NumPy's by a few ulp: the cases are
tests/test_augment_ref.py's NOISE_CASES, which that file shows to keep every value 1e-9 away from an integer before the truncation."""
import os
import random
import sys

import numpy as np
import pytest
import torch

import augment_ref as ar
import test_augment_ref as cpu

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
S = ar.step
SHAPES = ((28, 28), (13, 17), (4, 4), (64, 64))


@pytest.fixture(scope="module")
def aug():
    import sudoku_vision_amd as sva
    ml = os.path.join(os.path.dirname(sva.__file__), "ml")
    sys.path.insert(0, ml)
    try:
        sys.modules.pop("augment_data", None)
        import augment_data
    finally:
        sys.path.remove(ml)
    return augment_data


def gpu(ctx, src, chains, src_index=None, seed=0, index_base=0):
    steps, n_steps = ar.program(chains)
    si = np.zeros(len(chains), np.int32) if src_index is None else np.asarray(src_index, np.int32)
    out = ctx.augment(torch.from_numpy(src).to(ctx.device), steps, n_steps, si, seed=seed, index_base=index_base)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (steps, n_steps, si)


def check(ctx, src, chains, src_index=None, seed=0, index_base=0, what=""):
    got, (steps, n_steps, si) = gpu(ctx, src, chains, src_index, seed, index_base)
    want = ar.run_program(src, steps, n_steps, si, seed, index_base)
    bad = [o for o in range(len(chains)) if not (got[o] == want[o]).all()]
    assert not bad, f"{what}: outputs {bad[:8]} differ; first: ops {[int(s['op']) for s in chains[bad[0]]]}, {int((got[bad[0]] != want[bad[0]]).sum())} pixels"
    return got


def perspective(H, W, distortion, rs):
    src = np.float32([[0, 0], [W, 0], [W, H], [0, H]])
    dst = (src + rs.uniform(-distortion, distortion, (4, 2)).astype(np.float32) * np.float32([W, H])).astype(np.float32)
    return S(ar.PERSPECTIVE, d=ar.perspective_matrix(src, dst).reshape(9))


def single_steps(H, W):
    """Every step kind alone, at the parameters where it can go wrong: a list of (name, step)."""
    rs = np.random.RandomState(H * 100 + W)
    c = (W // 2, H // 2)
    out = [("rotate %g" % a, S(ar.AFFINE, d=ar.rotation_matrix(c, a).reshape(6))) for a in (0.0, 15.0, -15.0, 4.3, 90.0, 180.0)]
    # source coordinates on ties: the inverse of these forward matrices is exact, so (m1*y + b)*1024 and m3*x*1024 land on .5 at every
    # odd y resp. x (round half to even), and translations by odd multiples of 1/64 px put X0 + 16 on the boundary of the >> 5
    out += [("tie shear x", S(ar.AFFINE, d=[1, 1 / 2048, 1 / 64, 0, 1, 0])), ("tie shear y", S(ar.AFFINE, d=[1, 0, 0, 1 / 2048, 1, 3 / 64])),
            ("tie shift", S(ar.AFFINE, d=[1, 0, -5 / 64, 0, 1, 33 / 64])), ("singular", S(ar.AFFINE, d=[1, 2, 0, 2, 4, 0]))]
    mx, my = int(0.1 * W), int(0.1 * H)
    out += [("translate %d %d" % (dx, dy), S(ar.AFFINE, d=[1, 0, dx, 0, 1, dy])) for dx, dy in ((0, 0), (mx, my), (-mx, -my), (mx, -my), (W, 0), (0, -H))]
    out += [("perspective 0.1 #%d" % k, perspective(H, W, 0.1, rs)) for k in range(4)]
    out += [("perspective identity", S(ar.PERSPECTIVE, d=[1, 0, 0, 0, 1, 0, 0, 0, 1])), ("perspective singular", S(ar.PERSPECTIVE, d=[1, 2, 3, 2, 4, 6, 0, 0, 1]))]
    out += [("brightness %g" % d, S(ar.BRIGHTNESS, d=[d])) for d in (300.0, -300.0, -10.5, -0.25, 51.0, 50.7, 0.2 * 255)]
    out += [("contrast %g" % f, S(ar.CONTRAST, d=[f])) for f in (1.2, 0.8, 1.0, 3.7, -1.0)]
    out += [("blur %d" % k, S(ar.BLUR, i=[k])) for k in (1, 3, 5)]
    sizes = {(int(W * f), int(H * f), f > 1) for f in (0.9, 1.0, 1.1, 0.95, 1.05, 1.0999)} | {(W - 1, H - 3, False), (W + 1, H + 3, True), (W, H, True), (1, 1, False),
                                                                                             (2 * W, 2 * H, True), (W - 2, H, False), (W, H + 1, True)}
    out += [("scale %dx%d %s" % (nw, nh, crop), S(ar.SCALE, i=[nw, nh, int(crop)])) for nw, nh, crop in sorted(sizes) if nw >= 1 and nh >= 1]
    out += [("rect %s" % (r,), S(ar.FILL_RECT, i=list(r))) for r in ((0, 1, 2, 2, 255), (1, 0, 2, 1, 0), (W - 2, 1, 2, 2, 7), (1, H - 1, 2, 1, 200), (0, 0, W, H, 99),
                                                                  (0, 0, W, 1, 1), (0, 0, 1, H, 2), (2, 2, 0, 0, 5), (W - 1, H - 1, 1, 1, 128))]
    out += [("salt and pepper %g" % p, S(ar.NOISE_SP, i=[0, 0, 0, 0, 11], d=[p])) for p in (0.025, 0.5, 0.0, 1.0)]
    if min(H, W) >= 13:
        r, taps = ar.elastic_taps(3.0)
        out += [("elastic alpha %g" % a, S(ar.ELASTIC, i=[r, 0, 0, 0, salt], f=[a] + list(taps))) for a, salt in ((8.0, 1), (10.0, -2), (8.0, 3))]
    r1, taps1 = ar.elastic_taps(0.25)
    out += [("elastic sigma 0.25", S(ar.ELASTIC, i=[r1, 0, 0, 0, 4], f=[2.0] + list(taps1)))]
    return out


@pytest.mark.parametrize("H,W", SHAPES)
def test_each_step_alone(ctx, H, W):
    """One launch whose workgroups all run different one-step programs, on three images and a flat one."""
    src = np.concatenate([ar.sample_images(3, H, W, seed=H), np.full((1, H, W), 77, np.uint8)])
    named = single_steps(H, W)
    chains = [[s] for _, s in named] + [[S(ar.CONTRAST, d=[1.3])], [S(ar.CONTRAST, d=[0.7])]]
    src_index = [k % 3 for k in range(len(named))] + [3, 3]
    got = check(ctx, src, chains, src_index, seed=H * W, index_base=5, what=f"{H}x{W}")
    assert (got[-1] == 77).all() and (got[-2] == 77).all()                                   # a flat image keeps its value
    means = [float(src[k].astype(np.int64).sum()) / (H * W) for k in range(3)]
    assert any(m != int(m) for m in means)                                                   # the contrast steps saw a non-integer mean
    for (name, _), o, k in zip(named, got, src_index):
        if name in ("rotate 0", "translate 0 0", "perspective identity", "blur 1", "contrast 1", "salt and pepper 0") or name.startswith("scale %dx%d" % (W, H)):
            assert (o == src[k]).all(), name
        if name == "salt and pepper 1":
            assert (o == 0).all()
        if name.startswith("translate %d 0" % W):
            assert (o == src[k][:, :1]).all()                                                # shifted out: the replicated first column, not a constant


@pytest.mark.parametrize("n_out", [1, 3])
def test_zero_steps_is_a_copy(ctx, n_out):
    src = ar.sample_images(2, 13, 17)
    got = check(ctx, src, [[]] * n_out, [k % 2 for k in range(n_out)])
    assert (got == src[[k % 2 for k in range(n_out)]]).all()


def test_gaussian_noise_equals_the_reference(ctx):
    for seed, salt, H, W, sigma in cpu.NOISE_CASES:
        src = ar.sample_images(cpu.NOISE_N_OUT, H, W, seed)
        chains = [[S(ar.NOISE_GAUSS, i=[0, 0, 0, 0, salt], d=[sigma])]] * cpu.NOISE_N_OUT
        got = check(ctx, src, chains, list(range(cpu.NOISE_N_OUT)), seed=seed, index_base=1000, what=f"noise {H}x{W}")
        assert (got != src).mean() > 0.5


def test_salt_and_pepper_rates(ctx):
    src = np.full((3, 64, 64), 100, np.uint8)
    src[:, ::2] = 101
    got = check(ctx, src, [[S(ar.NOISE_SP, i=[0, 0, 0, 0, 9], d=[0.1])]] * 3, [0, 1, 2], seed=21)
    n, p = got.size, 0.1
    assert abs((got == 0).mean() - p) < 5 * np.sqrt(p * (1 - p) / n)                          # pepper goes over salt
    assert abs((got == 255).mean() - p * (1 - p)) < 5 * np.sqrt(p / n)


def ten_steps(H, W, salt):
    r, taps = ar.elastic_taps(3.0)
    rs = np.random.RandomState(salt)
    return [S(ar.AFFINE, d=ar.rotation_matrix((W // 2, H // 2), 11.0).reshape(6)), perspective(H, W, 0.1, rs), S(ar.BRIGHTNESS, d=[-20.4]), S(ar.CONTRAST, d=[1.15]),
            S(ar.BLUR, i=[5]), S(ar.NOISE_SP, i=[0, 0, 0, 0, salt], d=[0.02]), S(ar.ELASTIC, i=[r, 0, 0, 0, salt + 1], f=[8.0] + list(taps)),
            S(ar.AFFINE, d=[1, 0, 2, 0, 1, -1]), S(ar.SCALE, i=[int(W * 1.07), int(H * 1.07), 1]), S(ar.FILL_RECT, i=[3, 2, 5, 4, 250])]


def random_chain(rs, H, W):
    pool = ten_steps(H, W, int(rs.randint(1, 1000))) + [S(ar.NONE), S(ar.BLUR, i=[3]), S(ar.SCALE, i=[W - 3, H - 2, 0])]
    return [pool[k] for k in rs.permutation(len(pool))[:rs.choice([0, 1, 2, 3, 3, 3, 10])]]


@pytest.fixture(scope="module")
def many():
    """257 outputs of 5 images, every workgroup its own program: (src, chains, src_index, the reference's outputs)."""
    rs = np.random.RandomState(8)
    src = ar.sample_images(5, 28, 28, seed=3)
    chains = [ten_steps(28, 28, 5), ten_steps(28, 28, 6)[::-1]] + [random_chain(rs, 28, 28) for _ in range(255)]
    si = rs.randint(0, 5, 257).astype(np.int32)
    steps, n_steps = ar.program(chains)
    want = ar.run_program(src, steps, n_steps, si, seed=99, index_base=0)
    want.setflags(write=False)
    return src, chains, si, want


def test_257_different_programs(ctx, many):
    src, chains, si, want = many
    assert {len(c) for c in chains} >= {0, 1, 2, 3, 10}
    got, _ = gpu(ctx, src, chains, si, seed=99)
    bad = [o for o in range(257) if not (got[o] == want[o]).all()]
    assert not bad, f"outputs {bad[:8]} differ"


def test_split_calls_give_the_same_outputs(ctx, many):
    """A field depends on the global index, not on n_out or on how the job is cut."""
    src, chains, si, want = many
    a, _ = gpu(ctx, src, chains[:100], si[:100], seed=99, index_base=0)
    b, _ = gpu(ctx, src, chains[100:], si[100:], seed=99, index_base=100)
    assert (np.concatenate([a, b]) == want).all()
    c, _ = gpu(ctx, src, chains[:100], si[:100], seed=99, index_base=1)
    assert (c != want[:100]).any()


def test_ten_steps_at_the_ceiling_and_the_odd_shape(ctx):
    for H, W in ((64, 64), (13, 17)):
        src = ar.sample_images(2, H, W, seed=W)
        check(ctx, src, [ten_steps(H, W, 3), ten_steps(H, W, 4)[::-1], ten_steps(H, W, 5)[:3]], [0, 1, 1], seed=2 ** 63 + 5, index_base=2 ** 40, what=f"{H}x{W}")


def test_kernel_survives_what_the_check_refuses(ctx):
    """A device program is not checked: an unknown op is the identity, counts and indices are clamped, nothing is written elsewhere."""
    src = ar.sample_images(2, 28, 28)
    steps, n_steps = ar.program([[S(99), S(ar.BLUR, i=[7]), S(ar.ELASTIC, i=[40, 0, 0, 0, 0], f=[8.0])], [S(ar.FILL_RECT, i=[20, 20, 1000, 1000, 3])], []])
    n_steps[2] = 1000
    si = np.array([0, 5, -3], np.int32)
    raw = torch.from_numpy(steps.view(np.uint8).reshape(3, -1)).to(ctx.device)
    guard = torch.full((5, 28, 28), 171, dtype=torch.uint8, device=ctx.device)
    out = ctx.augment(torch.from_numpy(src).to(ctx.device), raw, torch.from_numpy(n_steps).to(ctx.device), torch.from_numpy(si).to(ctx.device), out=guard[1:4])
    torch.cuda.synchronize()
    got = guard.cpu().numpy()
    assert (got[0] == 171).all() and (got[4] == 171).all()
    assert (got[1] == src[0]).all() and (got[3] == src[0]).all()
    want = src[1].copy()
    want[20:, 20:] = 3
    assert (got[2] == want).all()


def test_refused_shapes(ctx):
    import sudoku_vision_amd as sva
    steps, n_steps = ar.program([[]])
    for shape in ((1, 3, 28), (1, 28, 65)):
        with pytest.raises(ValueError, match="4..64"):
            ctx.augment(torch.zeros(shape, dtype=torch.uint8, device=ctx.device), steps, n_steps, [0])
    with pytest.raises(sva._native.NativeError, match="source index 1"):
        ctx.augment(torch.zeros((1, 28, 28), dtype=torch.uint8, device=ctx.device), steps, n_steps, [1])


# ---- the drop-in ---------------------------------------------------------------------------------------------------------------
def seed_all(s):
    random.seed(s)
    np.random.seed(s)


def test_dropin_equals_the_golden_chains(ctx, aug):
    g = np.load(os.path.join(HERE, "golden", "augment_goldens.npz"))
    n = 0
    for c, seed, preset, image, n_aug in cpu.chains_of(g):
        if preset == "heavy":
            continue
        seed_all(seed)
        out = aug.augment_image(image, aug.create_augmentation_pipeline(preset), n_aug)
        assert isinstance(out, np.ndarray) and (out == g[f"c{c}_out"][-1]).all(), (c, seed, preset)
        seed_all(seed)
        batch, si = aug.augment_batch(image[None], 1, preset, n_aug)
        assert (batch[0] == out).all() and list(si) == [0]
        n += 1
    assert n == 16


@pytest.mark.parametrize("preset", ["medium", "heavy"])
def test_augment_batch_equals_the_loop(ctx, aug, preset):
    images = ar.sample_images(3, 28, 28, seed=12)
    seed_all(41)
    out, si = aug.augment_batch(torch.from_numpy(images).to(ctx.device), multiplier=4, intensity=preset, n_augmentations=4, seed=5)
    assert isinstance(out, torch.Tensor) and list(si) == [0] * 4 + [1] * 4 + [2] * 4
    seed_all(41)
    pipeline = aug.create_augmentation_pipeline(preset)
    loop = [aug.augment_image(images[n], pipeline, 4, seed=5, index=n * 4 + i) for n in range(3) for i in range(4)]
    assert (out.cpu().numpy() == np.stack(loop)).all()
    seed_all(41)
    steps, n_steps, si2 = aug.build_program(3, 28, 28, 4, aug.create_augmentation_pipeline(preset), 4)
    assert (out.cpu().numpy() == ar.run_program(images, steps, n_steps, si2, seed=5)).all()


def test_single_functions_and_foreign_callables(ctx, aug):
    img = ar.sample_image(28, 28, 2)
    seed_all(7)
    got = aug.rotate(img, (-15, 15))
    seed_all(7)
    angle = random.uniform(-15, 15)
    assert (got == ar.warp_affine(img, ar.rotation_matrix((14, 14), angle))).all()
    seed_all(8)
    got = aug.augment_image(img, [lambda im: 255 - im, aug.create_augmentation_pipeline("light")[1]], 2)
    seed_all(8)
    order = random.sample([0, 1], 2)
    want = img
    for k in order:
        want = 255 - want if k == 0 else ar.brightness(want, random.uniform(-0.1, 0.1) * 255)
    assert (got == want).all()
    with pytest.raises(ValueError, match="4..64"):
        aug.adjust_brightness(np.zeros((65, 28), np.uint8))
    seed_all(9)
    assert (aug.add_noise(img, "unknown") == img).all()


def test_process_directory(ctx, aug, tmp_path):
    from sudoku_vision_amd import imgcodecs as ic
    src, dst = tmp_path / "in", tmp_path / "out"
    shapes = {"0": (28, 28), "3": (13, 17), "10": (28, 28)}
    for label, (H, W) in shapes.items():
        (src / label).mkdir(parents=True)
        for k in range(3 if label != "10" else 1):
            assert ic.imwrite_png(str(src / label / f"cell_{k}.png"), ar.sample_image(H, W, seed=int(label) * 10 + k), ctx=ctx)
    (src / "notes").mkdir()
    seed_all(17)
    stats = aug.process_directory(src, dst, multiplier=2, intensity="medium")
    assert stats == {"originals": 7, "augmented": 14, "by_class": {"0": {"originals": 3, "augmented": 6}, "3": {"originals": 3, "augmented": 6},
                                                                   "10": {"originals": 1, "augmented": 2}}}
    seed_all(17)
    pipeline = aug.create_augmentation_pipeline("medium")
    for label in ("0", "3", "10"):                                                         # numeric order, as the reference sorts the classes
        files = list((src / label).glob("*.png")) + list((src / label).glob("*.jpg"))
        assert sorted(p.name for p in (dst / label).iterdir()) == sorted([f"orig_{f.name}" for f in files] + [f"aug_{i}_{f.name}" for f in files for i in range(2)])
        for f in files:
            img = ic.imread_png(str(f), ctx=ctx)[:, :, 0]
            assert (ic.imread_png(str(dst / label / f"orig_{f.name}"), ctx=ctx)[:, :, 0] == img).all()
            for i in range(2):
                steps, n_steps = ar.program([aug.draw_chain(*img.shape, pipeline)])
                want = ar.run_program(img[None], steps, n_steps, [0])[0]
                assert (ic.imread_png(str(dst / label / f"aug_{i}_{f.name}"), ctx=ctx)[:, :, 0] == want).all(), (label, f.name, i)
    assert not (dst / "notes").exists()
    with pytest.raises(ValueError, match="4..64"):
        (src / "5").mkdir()
        ic.imwrite_png(str(src / "5" / "big.png"), np.zeros((65, 65), np.uint8), ctx=ctx)
        aug.process_directory(src, tmp_path / "out2", multiplier=1)


# ---- stream order ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_jobs(ctx):
    """Two jobs of the same shape, A and B, with the reference's outputs: images, program, and all of it on the device."""
    rs = np.random.RandomState(4)
    jobs = {}
    for name in ("A", "B"):
        src = ar.sample_images(4, 28, 28, seed=rs.randint(1000))
        chains = [random_chain(rs, 28, 28) or [S(ar.BLUR, i=[3])] for _ in range(24)]
        si = rs.randint(0, 4, 24).astype(np.int32)
        steps, n_steps = ar.program(chains)
        want = ar.run_program(src, steps, n_steps, si, seed=6, index_base=10)
        dev = (torch.from_numpy(src).to(ctx.device),) + ctx.augment_upload_program(steps, n_steps, si, 4, 28, 28)
        jobs[name] = (dev, want)
    assert (jobs["A"][1] != jobs["B"][1]).any()
    return jobs


def test_on_a_busy_side_stream(ctx, two_jobs):
    """The call is enqueued behind a long kernel and late copies of job B over job A's buffers, with no synchronisation between."""
    bufs = [t.clone() for t in two_jobs["A"][0]]
    out = torch.zeros((24, 28, 28), dtype=torch.uint8, device=ctx.device)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(10_000_000)
        for b, t in zip(bufs, two_jobs["B"][0]):
            b.copy_(t, non_blocking=True)
        ctx.augment(bufs[0], bufs[1], bufs[2], bufs[3], seed=6, index_base=10, out=out)
    s.synchronize()
    assert (out.cpu().numpy() == two_jobs["B"][1]).all()
    torch.cuda.synchronize()


def test_captured_and_replayed_after_the_buffers_change(ctx, two_jobs):
    bufs = [t.clone() for t in two_jobs["A"][0]]
    out = torch.zeros((24, 28, 28), dtype=torch.uint8, device=ctx.device)
    ctx.augment(bufs[0], bufs[1], bufs[2], bufs[3], seed=6, index_base=10, out=out)               # warm-up: code objects
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g, stream=s):
            ctx.augment(bufs[0], bufs[1], bufs[2], bufs[3], seed=6, index_base=10, out=out)
    except Exception:
        torch.cuda.synchronize()
        raise
    for which in ("B", "A", "A"):
        for b, t in zip(bufs, two_jobs[which][0]):
            b.copy_(t, non_blocking=True)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == two_jobs[which][1]).all(), f"replay on {which}"
    del g
