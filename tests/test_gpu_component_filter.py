"""K11, the component filter (sv_component_filter_u8 / sv_component_filter_bits, csrc/k11_components.hip), against its restatement
tests/component_filter_ref.py, bit for bit: the smallest shapes, word and row boundaries, many components and one giant one, labels that
merge late, early and along one long chain, nesting, the threshold itself, rows wider than any band, batches, every form of the entry,
and the committed photos at full size.  Every comparison is an equality."""
import json
import os

import numpy as np
import pytest
import torch

import component_filter_ref as R
import despeckle_ref as D

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PHOTOS = json.load(open(os.path.join(GOLDEN, "cv_goldens.json")))["photos"]


def _want(imgs, r):
    return np.stack([R.component_filter(f, r) != 0 for f in imgs])


def _bytes(ctx, imgs, r, **kw):
    d = torch.from_numpy(np.asarray(imgs).astype(np.uint8) * 255).cuda()
    return ctx.component_filter(d, r, **kw).cpu().numpy() > 0


def _bits(ctx, imgs, r):
    W = imgs.shape[-1]
    got = ctx.component_filter_bits(torch.from_numpy(R.pack_bits(imgs)).cuda(), r)
    return R.unpack_bits(got.cpu().numpy(), W)


def _check(ctx, imgs, r):
    """Both entries (the bit one where the width allows) against the restatement."""
    imgs = np.asarray(imgs, bool)
    want = _want(imgs, r)
    assert np.array_equal(_bytes(ctx, imgs, r), want)
    if imgs.shape[-1] % 32 == 0:
        assert np.array_equal(_bits(ctx, imgs, r), want)
    return want


def _contents(shape):
    alt = np.zeros(shape, bool)
    alt[:, ::2] = True
    return np.stack([np.zeros(shape, bool), np.ones(shape, bool), alt])


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (5, 1), (1, 32), (1, 64), (3, 32)], ids=str)
@pytest.mark.parametrize("r", [0.0, 0.1, 1.0])
def test_smallest_shapes(ctx, shape, r):
    _check(ctx, _contents(shape), r)


def test_diagonal_joins_across_a_word_boundary(ctx):
    imgs = np.zeros((3, 2, 64), bool)
    imgs[0, 0, 31] = imgs[0, 1, 32] = True
    imgs[1, 0, 32] = imgs[1, 1, 31] = True
    imgs[2, 0, 63] = True
    for r in (1.0 / 128, 1.5 / 128):                      # floor 1.0: the joined pairs have box 1 x 1 and stay; floor 1.5: they go
        want = _check(ctx, imgs, r)
        assert want[:2].any() == (r < 0.01) and not want[2].any()


@pytest.mark.parametrize("shape,r", [((67, 61), 0.02), ((130, 250), 0.02), ((200, 96), 0.05)], ids=str)
def test_partial_last_word_and_three_words_per_row(ctx, shape, r):
    _check(ctx, np.stack([R.noise(0.3, 40 + f, shape) for f in range(3)]), r)


def _frames_192x288():
    H, W = 192, 288
    cases = {f"percolation {d}": np.stack([R.noise(d, int(d * 100) + f, (H, W)) for f in range(3)]) for d in (0.38, 0.5, 0.6)}
    cases["isolated"] = np.stack([R.isolated(H, W), R.isolated(H, W)[:, ::-1], R.isolated(H, W)[::-1]])
    cases["lattice"] = np.stack([R.lattice(H, W), ~R.lattice(H, W), R.lattice(H, W) & (np.arange(W) < 200)])
    cases["comb last"] = np.stack([R.comb(H, W), R.comb(H, W)[:, ::-1], R.comb(H, W) & (np.arange(W) > 40)])
    cases["comb first"] = np.stack([R.comb(H, W, "first"), R.comb(H, W, "first")[:, ::-1], R.comb(H, W, "first") & (np.arange(W) > 40)])
    cases["spiral"] = np.stack([R.frame_spiral(H, W), R.frame_spiral(H, W)[::-1], R.frame_spiral(H, W).T[:H, :].repeat(2, axis=1)[:, :W]])
    cases["rings"] = np.stack([R.rings(H, W), R.rings(H, W)[:, ::-1], R.rings(H, W)[::-1]])
    return cases


CASES_192 = _frames_192x288()


@pytest.mark.parametrize("name", list(CASES_192))
def test_192x288(ctx, name):
    imgs = CASES_192[name]
    want = _check(ctx, imgs, 0.1)
    if name == "isolated":
        assert not want.any()
    if name in ("lattice", "comb last", "comb first", "spiral"):
        assert np.array_equal(want[0], imgs[0])                              # one component, box = the frame: kept whole
    if name == "rings":
        assert want.any() and R.count_components(want[0]) == 1 and R.count_components(imgs[0]) == 4


def test_threshold_pair_192x288(ctx):
    frames, kept, under = R.threshold_frames(192, 288, 0.25)
    want = _check(ctx, frames, 0.25)
    assert kept[0] * kept[1] == 13824 == 0.25 * 192 * 288
    assert np.array_equal(want[0], frames[0]) and not want[1].any() and not want[2].any()


def test_rows_wider_than_any_band(ctx):
    imgs = np.stack([R.serpentine(70, 8192, s) for s in (1, 2)])
    want = _check(ctx, imgs, 0.1)
    assert R.count_components(imgs[0]) > 20 and R.count_components(want[0]) == 1


def test_topology_image(ctx):
    imgs = D.case_topology()[0]
    want = _check(ctx, imgs, 0.1)
    assert R.count_components(want[0]) == 1                                  # the outline


@pytest.mark.parametrize("shape", [(192, 288), (70, 8192)], ids=str)
def test_batch_independence(ctx, shape):
    imgs = D.case_independence(*shape)[0]
    assert len(imgs) == 5
    r = 0.002                                              # a floor that keeps some of the placed tiles and erases the specks
    want = _want(imgs[2:3], r)
    assert want.any() and (want != imgs[2:3]).any()
    alone = _bytes(ctx, imgs[2:3], r)
    assert np.array_equal(alone, want)
    assert np.array_equal(_bytes(ctx, imgs, r)[2], alone[0])
    assert np.array_equal(_bits(ctx, imgs, r)[2], alone[0])


def test_forms_agree_and_are_deterministic(ctx):
    imgs = np.stack([R.noise(0.5, 70 + f, (192, 288)) for f in range(3)])
    want = _want(imgs, 0.1)
    d = torch.from_numpy(imgs.astype(np.uint8) * 255).cuda()
    out = ctx.component_filter(d, 0.1)
    assert np.array_equal(out.cpu().numpy(), want.astype(np.uint8) * 255)     # kept pixels keep their value
    packed = torch.empty((3, 192, 9), dtype=torch.int32, device=d.device)
    out2 = torch.empty_like(d)
    assert ctx.component_filter(d, 0.1, out=out2, packed=packed) is out2
    assert torch.equal(out2, out) and np.array_equal(packed.cpu().numpy(), R.pack_bits(want))
    bits = ctx.component_filter_bits(torch.from_numpy(R.pack_bits(imgs)).cuda(), 0.1)
    assert torch.equal(bits, packed)
    again = ctx.component_filter_bits(torch.from_numpy(R.pack_bits(imgs)).cuda(), 0.1)
    assert torch.equal(again, bits)                                           # two runs, equal bits
    work = d.clone()
    assert ctx.component_filter(work, 0.1, out=work) is work and torch.equal(work, out)     # in place
    gray = torch.from_numpy((imgs * np.arange(1, 289, dtype=np.int64)[None, None, :] % 251 + imgs).astype(np.uint8)).cuda()
    got = ctx.component_filter(gray, 0.1).cpu().numpy()
    assert np.array_equal(got, np.stack([R.component_filter(g, 0.1) for g in gray.cpu().numpy()]))   # grey values survive where kept
    assert torch.equal(ctx.component_filter(d, 0.0), d)                       # ratio 0 erases nothing


def test_second_call_at_a_smaller_shape(ctx):
    big = np.stack([R.noise(0.45, 80, (300, 416))])
    small = np.stack([R.noise(0.45, 81, (67, 61)), R.noise(0.3, 82, (67, 61))])
    _check(ctx, big, 0.05)
    _check(ctx, small, 0.05)
    _check(ctx, big, 0.05)


def test_1080p(ctx):
    imgs = D.case_words(1080, 1920)[0]
    want = _check(ctx, imgs, 0.1)
    for f in range(3):
        assert R.count_components(want[f]) == 1 and R.count_components(imgs[f]) > 100


@pytest.mark.parametrize("rec", PHOTOS, ids=lambda r: r["file"])
def test_committed_photos(ctx, rec):
    """The K1 binary of every committed photo at full size, behind K4 (its precondition holds at this size) and K11: the restatement's
    bits, the unfiltered search's corners, the committed corners; and recognize_image(component_filter=True) == recognize_image()."""
    import sudoku_vision_amd as sva
    from sudoku_vision_amd import imgcodecs
    from sudoku_vision_amd.pipeline import recognize_image
    import cnn_oracle
    g2 = np.load(os.path.join(GOLDEN, "cnn_coreml_fp16.npz"))
    ctx.load_state_dict({k: torch.from_numpy(g2[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS})
    frame = imgcodecs.imread(os.path.join(GOLDEN, rec["file"]), device=True, ctx=ctx)
    H, W = frame.shape[:2]
    assert 0.1 * H * W > 61 * 61
    binary = ctx.preprocess(frame[None])
    k4 = ctx.despeckle(binary)
    got = ctx.component_filter(k4, 0.1)
    assert np.array_equal(got[0].cpu().numpy(), R.component_filter(k4[0].cpu().numpy(), 0.1))
    corners = sva.host.find_grid_corners(got[0].cpu().numpy())
    plain = sva.host.find_grid_corners(binary[0].cpu().numpy())
    as_list = lambda c: None if c is None else c.tolist()
    assert as_list(corners) == as_list(plain) == rec["corners"]
    a, b = recognize_image(frame, ctx=ctx, component_filter=True), recognize_image(frame, ctx=ctx)
    assert (a is None) == (b is None) == (rec["corners"] is None)
    if a is not None:
        assert set(a) == set(b) and a["grid"] == b["grid"] and (a["digits"] == b["digits"]).all() and (a["corners"] == b["corners"]).all()
        assert a["logits"].tobytes() == b["logits"].tobytes()


def test_bad_arguments(ctx):
    """In the style of tests/test_runtime_args.py: wrong kinds raise before the library sees a pointer."""
    from sudoku_vision_amd._native import NativeError
    ok = torch.zeros((1, 8, 64), dtype=torch.uint8, device=ctx.device)
    bits = torch.zeros((1, 8, 2), dtype=torch.int32, device=ctx.device)
    for call in (lambda: ctx.component_filter(ok.float()), lambda: ctx.component_filter(ok.cpu()), lambda: ctx.component_filter(ok[0]),
                 lambda: ctx.component_filter(ok, out=torch.zeros((1, 8, 32), dtype=torch.uint8, device=ctx.device)),
                 lambda: ctx.component_filter(ok, packed=torch.zeros((1, 8, 2), dtype=torch.uint8, device=ctx.device)),
                 lambda: ctx.component_filter_bits(bits.to(torch.int64)), lambda: ctx.component_filter_bits(bits.cpu()),
                 lambda: ctx.component_filter_bits(bits[0]), lambda: ctx.component_filter_bits(np.zeros((1, 8, 2), np.int32))):
        with pytest.raises((TypeError, ValueError)):
            call()
    for call in (lambda: ctx.component_filter(ok, -0.1), lambda: ctx.component_filter(ok, float("nan")), lambda: ctx.component_filter_bits(bits, -1.0),
                 lambda: ctx.component_filter(ok[:, :, :40].contiguous(), packed=torch.zeros((1, 8, 1), dtype=torch.int32, device=ctx.device))):
        with pytest.raises(ValueError):
            call()
    lib = ctx._lib                                                            # W % 32 != 0 for the bits form: the library's own error
    import ctypes as C
    rc = lib.sv_component_filter_bits(ctx._h, C.c_void_p(bits.data_ptr()), 1, 8, 40, 0.1, None)
    assert rc == -4
    with pytest.raises(NativeError, match="SV_ERR_UNSUPPORTED"):
        ctx._check(rc, "sv_component_filter_bits")
    with pytest.raises(NativeError, match="SV_ERR_BAD_ARG"):
        ctx._check(lib.sv_component_filter_bits(ctx._h, C.c_void_p(bits.data_ptr()), 1, 8, 64, -0.5, None), "sv_component_filter_bits")
    assert ctx.component_filter_bits(torch.zeros((0, 8, 2), dtype=torch.int32, device=ctx.device)).shape[0] == 0       # n == 0: a no-op
