"""GPU: the entries that share csrc/sv_device.h's cv2 arithmetic (sv_resize_px; sv_affine_invert, sv_affine_coord, sv_remap_split,
sv_remap_sample) agree with each other and with the numpy restatements, bit for bit, at the shapes where separate copies of that
arithmetic could drift apart: 1-wide and 1-high sources, upscaling (both border fix-ups on every row), exactly 2x either way.

Resize: Context.resize_linear (k_resize_linear), Context.motion_update (K15's small_px) and, where K22 takes the shape, a one-step
SV_AUG_SCALE program, all against warp_ref.resize.  K22 takes sources of 4..64 pixels a side and keeps the source's size: a smaller
result comes back centred in the pad value, a larger one as its centre crop, and the comparison is with the same placement of
warp_ref.resize's image.  18x26 -> 9x13 is the one shape where K15 takes its 2x2 area-mean form; warp_ref.resize has no branch for
it, but at exactly 2x its table is (offset 2d, weights 1024, 1024) on both axes, ((1024 * (((p00 + p01) * 1024) >> 4)) >> 16) is
p00 + p01 exactly, and so its result is (p00 + p01 + p10 + p11 + 2) >> 2: the area mean.  It is therefore the reference there too.

Affine: Context.warp_affine (K13's k_warp_affine) with border 0 and 77 against grid_v2_ref.warp_affine for every shape and matrix.
K22 and K23 refuse sides below 4, and K23's cells are square, so of the sources 1x1, 1x9, 9x1 and 5x4 only 5x4 can go through a
one-step SV_AUG_AFFINE program (K22, BORDER_REPLICATE: augment_ref.warp_affine), and none through K23.  A 5x5 source is added so that
K23's SV_SYN_AFFINE_CONST, which runs the same step with a constant border, is compared with synth_cells_ref.warp_affine_const at
the matching borders 0 and 77 on the very plane and matrix K13 and K22 get."""
import numpy as np
import pytest
import torch

import augment_ref as ar
import grid_v2_ref
import synth_cells_ref as sr
import warp_ref

pytestmark = pytest.mark.gpu

# (source h, w) -> (destination h, w)
RESIZES = [((1, 7), (1, 3)), ((7, 1), (3, 1)), ((1, 1), (4, 5)), ((2, 2), (5, 3)), ((3, 3), (64, 64)), ((40, 40), (28, 28)),
           ((9, 13), (18, 26)), ((18, 26), (9, 13))]
AFFINE_SHAPES = [(1, 1), (1, 9), (9, 1), (5, 4), (5, 5)]
BORDERS = [0, 77]
PAD = 128                                                 # what K22's scale step pads with


def _plane(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _matrices(H, W):
    return {"identity": np.array([[1, 0, 0], [0, 1, 0]], np.float64),
            "half-pixel shift": np.array([[1, 0, 0.5], [0, 1, 0.5]], np.float64),
            "rotation 33": grid_v2_ref.rotation_matrix(((W - 1) / 2, (H - 1) / 2), 33.0),
            "singular": np.array([[1, 2, 0.5], [2, 4, -1]], np.float64),
            "translation 40000": np.array([[1, 0, 40000], [0, 1, -40000]], np.float64)}


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and (got == want).all(), f"{what}: {int((got != want).sum())} of {want.size} bytes differ"


@pytest.mark.parametrize("src,dst", RESIZES, ids=lambda s: "%dx%d" % s)
def test_resize_entries_agree(ctx, src, dst):
    (sh, sw), (dh, dw) = src, dst
    img = _plane(src, 100 * sh + sw)
    want = warp_ref.resize(img, (dw, dh))
    _same(ctx.resize_linear(_dev(ctx, img), (dw, dh)), want, "resize_linear")
    small, counts = ctx.motion_update(_dev(ctx, img[None]), None, dsize=(dw, dh))
    _same(small[0], want, "motion_update")
    assert counts.cpu().numpy().tolist() == [0]
    if not (4 <= sh <= ar.MAX_SIDE and 4 <= sw <= ar.MAX_SIDE):
        return                                            # K22 refuses the source
    if dh <= sh and dw <= sw:
        placed = np.full(src, PAD, np.uint8)
        y0, x0 = (sh - dh) // 2, (sw - dw) // 2
        placed[y0:y0 + dh, x0:x0 + dw] = want
        crop = 0
    else:
        assert dh >= sh and dw >= sw
        y0, x0 = (dh - sh) // 2, (dw - sw) // 2
        placed = want[y0:y0 + sh, x0:x0 + sw]
        crop = 1
    steps, n_steps = ar.program([[ar.step(ar.SCALE, i=[dw, dh, crop])]])
    _same(ctx.augment(_dev(ctx, img[None]), steps, n_steps, np.zeros(1, np.int32))[0], placed, "augment scale")


@pytest.mark.parametrize("shape", AFFINE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_affine_entries_agree(ctx, shape):
    H, W = shape
    img = _plane(shape, 1000 + 100 * H + W)
    mats = _matrices(H, W)
    names = list(mats)
    M = np.stack([mats[k] for k in names])
    planes = _dev(ctx, np.repeat(img[None], len(names), 0))
    for border in BORDERS:
        got = ctx.warp_affine(planes, M, (W, H), border_value=border).cpu().numpy()
        for k, name in enumerate(names):
            _same(got[k], grid_v2_ref.warp_affine(img, M[k], (W, H), border), f"warp_affine {name} border {border}")
    if not (4 <= H <= ar.MAX_SIDE and 4 <= W <= ar.MAX_SIDE):
        return                                            # K22 and K23 refuse the source
    steps, n_steps = ar.program([[ar.step(ar.AFFINE, d=M[k].reshape(6))] for k in range(len(names))])
    got = ctx.augment(planes[:1], steps, n_steps, np.zeros(len(names), np.int32)).cpu().numpy()
    for k, name in enumerate(names):
        _same(got[k], ar.warp_affine(img, M[k]), f"augment affine {name}")
    if H != W:
        return                                            # K23's cells are square
    keep = sr.cells_array([sr.cell(sr.KEEP)] * len(names))
    atlas = sr.atlas_of([np.full((1, 1), 255, np.uint8)])
    for border in BORDERS:
        steps, n_steps = ar.program([[ar.step(sr.AFFINE_CONST, i=[border], d=M[k].reshape(6))] for k in range(len(names))])
        got = ctx.synth_cells(keep, steps, n_steps, H, atlas, out=planes.clone()).cpu().numpy()
        for k, name in enumerate(names):
            _same(got[k], sr.warp_affine_const(img, M[k], border), f"synth affine {name} border {border}")
