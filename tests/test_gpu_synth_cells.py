"""GPU: K23 (sv_synth_cells_u8, Context.synth_cells) and the ml/generate_synthetic_v2.py drop-in, bit for bit against
tests/synth_cells_ref.py.

Sizes: 28; 12, where a size-24 glyph overhangs all four sides and its origin is negative; 64, the ceiling; 4 for base images alone; n_out
of 1 and 257.  The Gaussian fields are compared for equality although the device's ln and cos may differ from NumPy's by a few ulp: the
cases are tests/test_synth_cells_ref.py's FIELD_CASES and seeded batch, which that file shows to keep every value 1e-9 away from an
integer before the truncation."""
import json
import os
import random

import numpy as np
import pytest
import torch

import augment_ref as ar
import synth_cells_ref as sr
import test_synth_cells_ref as cpu

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
S, cell = ar.step, sr.cell
MASKS = [sr.sample_mask(18, 11, 1), sr.sample_mask(20, 15, 2), sr.sample_mask(32, 32, 3), np.full((1, 1), 255, np.uint8), np.zeros((5, 7), np.uint8)]
ATLAS = sr.atlas_of(MASKS)


@pytest.fixture(scope="module")
def gen():
    return cpu.load_dropin()


def gpu(ctx, cells, chains, size, seed=0, index_base=0, atlas=ATLAS):
    steps, n_steps = ar.program(chains)
    out = ctx.synth_cells(sr.cells_array(cells), steps, n_steps, size, atlas, seed=seed, index_base=index_base)
    torch.cuda.synchronize()
    return out.cpu().numpy(), steps, n_steps


def check(ctx, cells, chains, size, seed=0, index_base=0, what=""):
    got, steps, n_steps = gpu(ctx, cells, chains, size, seed, index_base)
    want = sr.run_job(sr.cells_array(cells), steps, n_steps, size, ATLAS, seed, index_base)
    bad = [o for o in range(len(cells)) if not (got[o] == want[o]).all()]
    assert not bad, f"{what}: outputs {bad[:8]} differ; first: ops {[int(s['op']) for s in chains[bad[0]]]}, {int((got[bad[0]] != want[bad[0]]).sum())} pixels"
    return got


def backgrounds(size):
    """Every background kind alone (no Gaussian field: those are FIELD_CASES), with artefacts and smudges at their edges."""
    out = [cell(sr.PLAIN, v) for v in (235, 255, 0)]
    for strength in (3.0, 9.99, 7.123456789):
        out += [cell(sr.GRADIENT, 240, grad_dir=d, bg_d=sr.linspace_terms(strength, size)) for d in (0, 1)] + [cell(sr.GRADIENT, 250, grad_dir=2, bg_d=[strength])]
    out += [cell(sr.GRADIENT, 254, grad_dir=0, bg_d=sr.linspace_terms(300.0, size)), cell(sr.GRADIENT, 3, grad_dir=2, bg_d=[10.0])]            # both clips
    out += [cell(sr.PLAIN, 250, art=(bits, w, 200)) for bits in (1, 2, 4, 8, 15, 5) for w in (1, 2)]
    out += [cell(sr.GRADIENT, 245, grad_dir=1, bg_d=sr.linspace_terms(8.0, size), art=(15, 2, 180), smudge=(size - 2, 0, 2, 210)),
            cell(sr.PLAIN, 250, smudge=(0, size - min(5, size), min(5, size), 240)), cell(sr.PLAIN, 200, smudge=(1, 1, 2, 230))]
    return out


def glyphs(size):
    """Placement: wholly outside, clipped at each side, ink 0 and 30, masks with 0 and 255, the full 32 x 32 slot."""
    spots = [(-40, 3), (3, size), (size, 0), (0, -33), (-5, 2), (size - 4, 2), (2, -7), (2, size - 3), (1, 1), (-3, -4)]
    out = [cell(sr.PLAIN, 250, glyph=(k % 3, x, y, ink)) for k, (x, y) in enumerate(spots) for ink in (0, 30)]
    out += [cell(sr.GRADIENT, 247, grad_dir=2, bg_d=[6.5], glyph=(3, size // 2, size // 2, 0)), cell(sr.PLAIN, 251, glyph=(4, 0, 0, 0)), cell(sr.PLAIN, 255, glyph=(2, -2, -2, 17))]
    return out


def new_ops(size):
    c = (size // 2, size // 2)
    rs = np.random.RandomState(size)
    out = [("rotate %g" % a, S(sr.AFFINE_CONST, i=[255], d=ar.rotation_matrix(c, a).reshape(6))) for a in (10.0, -10.0, 8.0, 0.0, 45.0)]
    out += [("rotate border 0", S(sr.AFFINE_CONST, i=[0], d=ar.rotation_matrix(c, 7.0).reshape(6))), ("shift out", S(sr.AFFINE_CONST, i=[255], d=[1, 0, size, 0, 1, 0]))]
    src = np.float32([[0, 0], [size, 0], [size, size], [0, size]])
    for k in range(3):
        u = rs.uniform(0, 2.5, 8)
        dst = np.float32([[u[0], u[1]], [size - u[2], u[3]], [size - u[4], size - u[5]], [u[6], size - u[7]]])
        out.append(("perspective #%d" % k, S(sr.PERSPECTIVE_CONST, i=[255 if k else 9], d=ar.perspective_matrix(src, dst).reshape(9))))
    out += [("scale %d" % n, S(sr.SCALE_PAD, i=[n, n, int(n > size), 255])) for n in sorted({1, 2, int(size * 0.9), size - 1, size, size + 1, int(size * 1.1), size + 6})]
    out += [("scale pad 7", S(sr.SCALE_PAD, i=[size - 3, size - 2, 0, 7]))]
    out += [("blur %d %g" % (k, s), S(sr.GAUSS_BLUR, i=[k] + sr.gaussian_taps_q8(k, s))) for k in (3, 5) for s in (0.3, 1.0, 0.65)]
    out += [("erode", S(sr.ERODE)), ("dilate", S(sr.DILATE))]
    return out


@pytest.mark.parametrize("size", [28, 12, 64, 4])
def test_base_images(ctx, size):
    cells = backgrounds(size) + glyphs(size)
    got = check(ctx, cells, [[]] * len(cells), size, what=f"base {size}")
    assert (got[0] == 235).all() and (got[len(backgrounds(size))] == 250).all()             # plain; a glyph wholly outside draws nothing
    assert any((g != g[0, 0]).any() for g in got[len(backgrounds(size)):])


@pytest.mark.parametrize("size", [28, 12, 64])
def test_each_new_op_alone(ctx, size):
    """One launch whose workgroups all run different one-step programs on a glyph cell, plus the morphology ops on a checkerboard (a
    plain cell under a period-1 mask) whose taps reach the image edge."""
    named = new_ops(size)
    base = cell(sr.GRADIENT, 246, grad_dir=0, bg_d=sr.linspace_terms(9.0, size), glyph=(1, size // 2 - 8, size // 2 - 11, 12))
    y, x = np.mgrid[0:32, 0:32]
    board = sr.atlas_of(MASKS[:4] + [(((x + y) & 1) * 255).astype(np.uint8)])
    cells = [base] * len(named) + [cell(sr.PLAIN, 250, glyph=(4, -1, -1, 0))] * 2
    chains = [[s] for _, s in named] + [[S(sr.ERODE)], [S(sr.DILATE)]]
    steps, n_steps = ar.program(chains)
    out = ctx.synth_cells(sr.cells_array(cells), steps, n_steps, size, board, seed=size)
    torch.cuda.synchronize()
    got, want = out.cpu().numpy(), sr.run_job(sr.cells_array(cells), steps, n_steps, size, board, size)
    for k, (name, _) in enumerate(named):
        assert (got[k] == want[k]).all(), (size, name, int((got[k] != want[k]).sum()))
    assert (got[-2] == want[-2]).all() and (got[-1] == want[-1]).all()
    plain = sr.base_image(base, size, board)
    by_name = {name: got[k] for k, (name, _) in enumerate(named)}
    assert (by_name["rotate 0"] == plain).all() and (by_name["scale %d" % size] == plain).all()
    assert (by_name["shift out"] == 255).all() and (by_name["rotate 45"][0, 0] == 255) and (by_name["rotate border 0"] < 100).any()
    assert (by_name["scale 1"] == 255).sum() == size * size - 1
    m = min(size, 31)                                           # the board covers 31 x 31 from the origin; pixel (0, 0) has no neighbour and is white
    assert (got[-2][1:m, 1:m] == 0).all() and got[-2][0, 0] == 250 and (got[-1][:m, :m] == 250).all()


def test_gaussian_fields_equal_the_reference(ctx):
    for (seed, salt, size, base, sigma, kind) in cpu.FIELD_CASES:
        cells = [c for s, _, _, c in cpu.field_cells() if s == seed]
        got = check(ctx, cells, [[]] * len(cells), size, seed=seed, index_base=cpu.FIELD_BASE, what=f"field {size}")
        assert len(np.unique(got)) > 4 and (got[0] != got[1]).any()


@pytest.fixture(scope="module")
def many(gen):
    """257 different cells (the seeded batch of the CPU file, cycled with other salts through index) with their reference outputs."""
    cpu.seed_all(cpu.BATCH_SEED)
    fonts = [("ring", cpu.RingFont())]
    cells, steps, n_steps, atlas = gen.build_cells(cpu.BATCH_LABELS, fonts, 28)
    n = len(cells)
    idx = [k % n for k in range(257)]
    cells, steps, n_steps = cells[idx], steps[idx], n_steps[idx]
    for o in range(n, 257):                                    # later copies lose their Gaussian fields: only outputs < n were vetted
        if cells[o]["bg_kind"] in (sr.TEXTURED, sr.NOISY):
            cells[o]["bg_kind"], cells[o]["grain_stride"] = sr.PLAIN, 0
        for k in range(n_steps[o]):
            if steps[o, k]["op"] == ar.NOISE_GAUSS:
                steps[o, k] = S(ar.BLUR, i=[3])
        cells[o]["bg_value"] = 200 + o % 56
    want = sr.run_job(cells, steps, n_steps, 28, atlas, cpu.BATCH_FIELD_SEED)
    want.setflags(write=False)
    return cells, steps, n_steps, atlas, want


def test_257_different_cells(ctx, many):
    cells, steps, n_steps, atlas, want = many
    out = ctx.synth_cells(cells, steps, n_steps, 28, atlas, seed=cpu.BATCH_FIELD_SEED)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    bad = [o for o in range(257) if not (got[o] == want[o]).all()]
    assert not bad, f"outputs {bad[:8]} differ"


def test_split_calls_give_the_same_outputs(ctx, many):
    """A field depends on the global index, not on n_out or on how the job is cut."""
    cells, steps, n_steps, atlas, want = many
    a = ctx.synth_cells(cells[:20], steps[:20], n_steps[:20], 28, atlas, seed=cpu.BATCH_FIELD_SEED, index_base=0)
    b = ctx.synth_cells(cells[20:], steps[20:], n_steps[20:], 28, atlas, seed=cpu.BATCH_FIELD_SEED, index_base=20)
    torch.cuda.synchronize()
    assert (np.concatenate([a.cpu().numpy(), b.cpu().numpy()]) == want).all()
    c = ctx.synth_cells(cells[:20], steps[:20], n_steps[:20], 28, atlas, seed=cpu.BATCH_FIELD_SEED, index_base=1)
    assert (c.cpu().numpy() != want[:20]).any()


def test_kernel_survives_what_the_check_refuses(ctx):
    """A device job is not checked: a bad slot draws nothing, offsets, counts and taps are clamped, an unknown op is the identity, and nothing
    is written outside the output.  tools/dev/synth_program_ubsan.cpp runs these records through the same functions on the CPU."""
    imax, imin = 2 ** 31 - 1, -2 ** 31
    bad_slot = cell(sr.PLAIN, 250, glyph=(7, 0, 0, 0))
    huge = cell(sr.PLAIN, 1000, glyph=(0, imin, imax, imin), smudge=(imin, imin, imax, imin), art=(imax, imax, imax))
    lying = cell(sr.PLAIN, 240, glyph=(1, -3, -3, 30))
    cells = sr.cells_array([bad_slot, huge, lying])
    steps, n_steps = ar.program([[S(99), S(sr.GAUSS_BLUR, i=[9, 1, 1, 1])], [], [S(sr.ERODE)]])
    n_steps[1] = 1000
    dims = np.array([[11, 18], [1000000, -5]], np.int32)
    atlas = np.full((2, 32, 32), 200, np.uint8)
    dev = lambda a: torch.from_numpy(a).to(ctx.device)
    guard = torch.full((5, 28, 28), 171, dtype=torch.uint8, device=ctx.device)
    ctx.synth_cells(dev(cells.view(np.uint8).reshape(3, -1)), dev(steps.view(np.uint8).reshape(3, -1)), dev(n_steps), 28, (dev(atlas), dev(dims)), out=guard[1:4])
    torch.cuda.synchronize()
    got = guard.cpu().numpy()
    assert (got[0] == 171).all() and (got[4] == 171).all()
    assert (got[1] == 250).all()                                                        # no glyph, identity steps
    assert (got[2] == 255).all()                                                        # value clamped to 255; width clamped to 2 with darkness 255; the smudge is off the cell
    assert (got[3] == 240).all()                                                        # a height of -5 clamps to 0: nothing is drawn


def test_refused_arguments(ctx):
    import sudoku_vision_amd as sva
    steps, n_steps = ar.program([[]])
    for size in (3, 65):
        with pytest.raises(ValueError, match="4..64"):
            ctx.synth_cells(sr.cells_array([cell()]), steps, n_steps, size, ATLAS)
    with pytest.raises(sva._native.NativeError, match="glyph_slot: 5"):
        ctx.synth_cells(sr.cells_array([cell(glyph=(5, 0, 0, 0))]), steps, n_steps, 28, ATLAS)


# ---- stream order ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_jobs(ctx, many):
    cells, steps, n_steps, atlas, want = many
    jobs = {}
    for name, sl in (("A", slice(0, 24)), ("B", slice(24, 48))):
        w = sr.run_job(cells[sl], steps[sl], n_steps[sl], 28, atlas, seed=6, index_base=10)
        c, s, n, (a, d) = ctx.synth_upload_program(cells[sl], steps[sl], n_steps[sl], 28, atlas)
        jobs[name] = ((c, s, n, a, d), w)
    assert (jobs["A"][1] != jobs["B"][1]).any()
    return jobs


def _vetted(many):
    """Outputs 0..47 at index_base 10 under seed 6 are not the vetted fields: keep only cells without a Gaussian field for equality."""
    cells, steps, n_steps, *_ = many
    return np.array([cells[o]["bg_kind"] not in (sr.TEXTURED, sr.NOISY) and not any(steps[o, k]["op"] == ar.NOISE_GAUSS for k in range(n_steps[o])) for o in range(48)])


def test_on_a_busy_side_stream(ctx, two_jobs, many):
    """The call is enqueued behind a long kernel and late copies of job B over job A's buffers, with no synchronisation between."""
    keep = _vetted(many)[24:48]
    bufs = [t.clone() for t in two_jobs["A"][0]]
    out = torch.zeros((24, 28, 28), dtype=torch.uint8, device=ctx.device)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(10_000_000)
        for b, t in zip(bufs, two_jobs["B"][0]):
            b.copy_(t, non_blocking=True)
        ctx.synth_cells(bufs[0], bufs[1], bufs[2], 28, (bufs[3], bufs[4]), seed=6, index_base=10, out=out)
    s.synchronize()
    assert keep.sum() >= 8 and (out.cpu().numpy()[keep] == two_jobs["B"][1][keep]).all()
    torch.cuda.synchronize()


def test_captured_and_replayed_after_the_buffers_change(ctx, two_jobs, many):
    vetted = _vetted(many)
    bufs = [t.clone() for t in two_jobs["A"][0]]
    out = torch.zeros((24, 28, 28), dtype=torch.uint8, device=ctx.device)
    ctx.synth_cells(bufs[0], bufs[1], bufs[2], 28, (bufs[3], bufs[4]), seed=6, index_base=10, out=out)     # warm-up: code objects
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g, stream=s):
            ctx.synth_cells(bufs[0], bufs[1], bufs[2], 28, (bufs[3], bufs[4]), seed=6, index_base=10, out=out)
    except Exception:
        torch.cuda.synchronize()
        raise
    for which in ("B", "A", "A"):
        for b, t in zip(bufs, two_jobs[which][0]):
            b.copy_(t, non_blocking=True)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        keep = vetted[:24] if which == "A" else vetted[24:48]
        assert (out.cpu().numpy()[keep] == two_jobs[which][1][keep]).all(), f"replay on {which}"
    del g


# ---- the drop-in -----------------------------------------------------------------------------------------------------------------
def test_generate_batch_equals_the_loop_of_single_calls(ctx, gen, many):
    fonts = [("ring", cpu.RingFont())]
    cpu.seed_all(cpu.BATCH_SEED)
    out = gen.generate_batch(cpu.BATCH_LABELS, fonts, 28, seed=cpu.BATCH_FIELD_SEED)
    assert isinstance(out, torch.Tensor) and out.is_cuda and tuple(out.shape) == (len(cpu.BATCH_LABELS), 28, 28)
    got = out.cpu().numpy()
    assert (got == many[4][:len(cpu.BATCH_LABELS)]).all()                             # = the restatement of build_cells' job
    cpu.seed_all(cpu.BATCH_SEED)
    for n, label in enumerate(cpu.BATCH_LABELS):
        kw = dict(seed=cpu.BATCH_FIELD_SEED, index=n)
        img = gen.generate_empty_cell(28, **kw) if label == 0 else gen.generate_digit(label, gen.pick_font(fonts), 28, 2, **kw)
        img = gen.apply_augmentation(img, is_empty=(label == 0), **kw)
        assert isinstance(img, np.ndarray) and (img == got[n]).all(), (n, label)


def test_single_functions(ctx, gen):
    cpu.seed_all(21)
    bg = gen.generate_paper_background(28)
    assert bg.shape == (28, 28) and bg.dtype == np.uint8 and bg.min() > 200
    cpu.seed_all(22)
    got = gen.add_grid_artifacts(bg)
    cpu.seed_all(22)
    dark, width = random.randint(180, 220), random.randint(1, 2)
    edges = sum(bit for bit in (1, 2, 4, 8) if random.random() > 0.6)
    assert (got == sr.artefacts(bg, edges, width, dark)).all()
    with pytest.raises(ValueError, match="4..64"):
        gen.generate_empty_cell(65)


def test_golden_cells_come_out_byte_identical(ctx, gen):
    """Where the reference's output is its own arithmetic (no np.random field: plain and gradient papers, artefacts, smudge, the glyph blend,
    brightness, contrast, pad / crop) and the stated cv2 contract, the drop-in's cells are the golden bytes."""
    g = np.load(os.path.join(HERE, "golden", "synth_cells_goldens.npz"))
    bases = wholes = 0
    for c, label, size, whole, bg_normals, cells, steps, n_steps, atlas in cpu.golden_jobs(gen, g):
        if bg_normals:
            continue
        base = ctx.synth_cells(cells, steps, np.zeros(1, np.int32), size, atlas).cpu().numpy()[0]
        assert (base == g[f"c{c}_base"]).all(), c
        bases += 1
        if whole:
            assert (ctx.synth_cells(cells, steps, n_steps, size, atlas).cpu().numpy()[0] == g[f"c{c}_out"]).all(), c
            wholes += 1
    assert bases >= 10 and wholes >= 4


def test_generate_dataset(ctx, gen, tmp_path):
    from sudoku_vision_amd import imgcodecs as ic
    fonts = [("ring", cpu.RingFont())]
    meta = gen.generate_dataset(tmp_path / "ds", num_per_class=5, val_ratio=0.2, size=28, seed=9, fonts=fonts)
    assert set(meta) == {"size", "num_per_class", "val_ratio", "seed", "stats"} and meta == json.load(open(tmp_path / "ds" / "metadata.json"))
    st = meta["stats"]
    assert set(st) == {"total_generated", "train_count", "val_count", "per_class", "fonts_used"}
    assert (st["total_generated"], st["train_count"], st["val_count"], st["fonts_used"]) == (50, 40, 10, ["ring"])
    assert st["per_class"] == {str(d): {"train": 4, "val": 1} for d in range(10)}
    cpu.seed_all(9)
    random.randint(18, 24)
    for digit in range(10):
        assert sorted(p.name for p in (tmp_path / "ds" / "val" / str(digit)).iterdir()) == [f"{digit}_000000.png"]
        assert sorted(p.name for p in (tmp_path / "ds" / "train" / str(digit)).iterdir()) == [f"{digit}_{i:06d}.png" for i in range(1, 5)]
        cells, steps, n_steps, atlas = gen.build_cells([digit] * 5, fonts, 28)
        batch = ctx.synth_cells(cells, steps, n_steps, 28, atlas, seed=9, index_base=digit * 5).cpu().numpy()
        for i in range(5):
            img = ic.imread_png(str(tmp_path / "ds" / ("val" if i < 1 else "train") / str(digit) / f"{digit}_{i:06d}.png"), ctx=ctx)
            assert (img[:, :, 0] == batch[i]).all(), (digit, i)
    assert sorted(p.name for p in (tmp_path / "ds").iterdir()) == ["metadata.json", "train", "val"]
