"""K4, the speck filter, where its flood fill turns or gives up: sv_despeckle_u8 (out of place, in place, with `packed`) and
sv_despeckle_bits against tests/despeckle_ref.py, pixel for pixel, on tiles that need 50...64 fill iterations (the alternation runs long),
on tiles that need more iterations than the kernel allows itself (left untouched for that pass), at layouts the byte and bit kernels index
differently, and across the frames of a batch.  tests/test_despeckle_ref.py proves on the CPU that every input is in its regime."""
import numpy as np
import pytest
import torch

import despeckle_ref as R

pytestmark = pytest.mark.gpu


def _unpack(bits, n, H):
    return np.unpackbits(bits.cpu().numpy().view(np.uint8).reshape(n, H, -1), axis=2, bitorder="little").astype(bool)


def _forms(ctx, imgs, byte_forms=True):
    """imgs bool [n,H,W] -> {form: result bool [n,H,W]} for every form of the filter the shape allows."""
    n, H, W = imgs.shape
    out = {}
    if byte_forms:
        d = torch.from_numpy(imgs.astype(np.uint8) * 255).cuda()
        keep = d.clone()
        out["out of place"] = ctx.despeckle(d).cpu().numpy() > 0
        assert torch.equal(d, keep)                                          # the input is not written
        work = d.clone()
        ctx.despeckle(work, out=work)
        out["in place"] = work.cpu().numpy() > 0
    if W % 32 == 0:
        if byte_forms:
            packed = torch.full((n, H, W // 32), -1, dtype=torch.int32, device="cuda")
            ctx.despeckle(d, out=torch.empty_like(d), packed=packed)
            out["packed"] = _unpack(packed, n, H)
        bits = torch.from_numpy(np.packbits(imgs, axis=2, bitorder="little").view(np.int32)).cuda()
        out["bits"] = _unpack(ctx.despeckle_bits(bits), n, H)
    return out


def _where(a, b):
    ys, xs = np.nonzero(a != b)
    return f"{len(ys)} px differ, first at (y={ys[0]}, x={xs[0]}), tile of the first grid ({ys[0] // 64}, {xs[0] // 64})" if len(ys) else "equal"


def _check_exact(ctx, imgs, byte_forms=True):
    """Every form equals the reference on every frame; the reference must be sure of every tile.  -> (forms, [(want, hard)])"""
    forms = _forms(ctx, imgs, byte_forms)
    refs = []
    for f, img in enumerate(imgs):
        want, hard, unsure = R.despeckle(img)
        assert unsure == [], (f, unsure)
        for name, got in forms.items():
            assert np.array_equal(got[f], want), (name, f, _where(got[f], want))
        refs.append((want, hard))
    return forms, refs


def _check_search(ctx, imgs, filtered, ratios=(0.1, 0.02)):
    """The claim: the host corner search finds on the filtered image (bytes, bits, sparse records) what it finds on the raw one.
    -> number of (frame, ratio) pairs with a grid."""
    import sudoku_vision_amd as sva
    n, H, W = imgs.shape
    raw = imgs.astype(np.uint8) * 255
    bits = torch.from_numpy(np.packbits(filtered, axis=2, bitorder="little").view(np.int32)).cuda()
    stride = sva.host.sparse_bits_record_bytes(H, W, H * (W // 32))              # room for every word: dense noise overflows less
    recs = ctx.pack_sparse_bits(bits, torch.empty((n, stride), dtype=torch.uint8, device="cuda")).cpu().numpy()
    found = 0
    for ratio in ratios:
        assert ratio * H * W > 61 * 61                                       # the filter's precondition
        cb, fb = sva.host.find_grid_corners_bits_batch(bits.cpu().numpy(), H, W, ratio, 0.02, 2)
        cs, fs = sva.host.find_grid_corners_sparse_batch(recs, H, W, ratio, 0.02, 2)
        for i in range(n):
            want = sva.host.find_grid_corners(raw[i], ratio)
            got = sva.host.find_grid_corners(filtered[i].astype(np.uint8) * 255, ratio)
            assert (want is None) == (got is None) and (want is None or (want == got).all()), (i, ratio)
            assert bool(fb[i]) == (want is not None) and (want is None or (cb[i] == want).all()), (i, ratio)
            assert fs[i] in (0, 1) and bool(fs[i]) == (want is not None) and (want is None or (cs[i] == want).all()), (i, ratio)
            found += want is not None
    return found


def test_capped_and_long_tiles(ctx):
    """Capped paths in all four orientations in tiles of both grids, each with a lone 3x3 speck in the same tile; long paths, spirals and
    noise tiles (50...64 iterations) and easy tiles beside them.  A capped tile comes through its pass untouched -- the speck survives
    that pass, and since it lies across a tile edge of the other grid it survives the filter -- and every other tile is filtered as the
    labelling says.  A rectangle outline runs through capped and long tiles of both grids; the search finds it, filtered or not."""
    imgs, tiles = R.case_topology()
    forms, refs = _check_exact(ctx, imgs)
    want, hard = refs[0]
    assert {p for p, _, _ in hard} == {0, 1} and len(hard) == 8
    full = R.despeckle(imgs[0], cap=None)[0]
    saved = want & ~full
    assert saved.any()                                                       # speck pixels that only the give-up path keeps ...
    for name, got in forms.items():
        assert (got[0] & saved).sum() == saved.sum() == 8 * 9, name          # ... and the kernels keep them
        for p, y0, x0 in hard:
            if p == 1:                                                       # nothing runs after the second pass: the tile is as it went in
                assert (got[0][y0:y0 + 64, x0:x0 + 64] & ~full[y0:y0 + 64, x0:x0 + 64]).sum() == 9, (name, y0, x0)
    assert _check_search(ctx, imgs, forms["bits"]) == 2


@pytest.mark.parametrize("shape", ["130x250", "67x61"])
def test_byte_kernel_slow_path_three_frames(ctx, shape):
    """W % 4 != 0: every tile of the byte kernel reads and writes pixel by pixel; H % 64 != 0 and three different frames: the tile ->
    frame arithmetic.  (130, 250) with capped and long tiles, (67, 61) -- one clipped tile per pass and side -- with density-0.3 noise."""
    imgs, _ = R.case_bytes_odd()[0 if shape == "130x250" else 1]
    assert imgs.shape[2] % 4 and imgs.shape[1] % 64
    forms, refs = _check_exact(ctx, imgs)
    assert set(forms) == {"out of place", "in place"}
    assert any(hard for _, hard in refs) == (shape == "130x250")


@pytest.mark.parametrize("H,W", [(200, 96), (1080, 1920)])
def test_three_frames_all_forms(ctx, H, W):
    """Three different frames through the byte, packed and bit forms: (200, 96) is W % 64 == 32 with an odd number of words per row in the
    band kernel; (1080, 1920) the production shape, with capped and long tiles at other places in every frame and a rectangle outline
    through some of them."""
    imgs, _ = R.case_words(H, W)
    forms, refs = _check_exact(ctx, imgs)
    assert set(forms) == {"out of place", "in place", "packed", "bits"}
    assert all(hard for _, hard in refs)
    if H == 1080:
        assert all({p for p, _, _ in hard} == {0, 1} for _, hard in refs)
        assert _check_search(ctx, imgs, forms["bits"]) == 6


def test_tile_per_wave_kernel(ctx):
    """(70, 8192), two frames: too wide for the band kernel, so sv_despeckle_bits runs k_despeckle_bits (TPW tiles per wave).  Capped
    and long tiles in the first and last tile of a tile row and either side of a boundary between two waves' groups, in both grids."""
    imgs, _ = R.case_strip()
    forms, refs = _check_exact(ctx, imgs)
    assert set(forms) == {"out of place", "in place", "packed", "bits"}
    assert all({p for p, _, _ in hard} == {0, 1} for _, hard in refs)
    # the search on this shape: a frame with an outline well inside it, filtered by the tile-per-wave kernel
    H, W = imgs.shape[1:]
    framed = imgs | R.rectangle_outline(H, W, 3, 64, 64 * 20 + 3, 64 * 40 + 3)[None]
    filtered = _forms(ctx, framed, byte_forms=False)["bits"]
    assert not (filtered & ~framed).any() and (framed & ~filtered).any()
    assert _check_search(ctx, framed, filtered) >= 2


@pytest.mark.parametrize("H,W", [(192, 288), (70, 8192)])
def test_frames_are_independent(ctx, H, W):
    """Five frames; only frame 2 holds capped and long tiles, its neighbours hold easy specks in the same tiles.  Every frame of the batch
    equals the result of filtering it alone (and the reference): nothing of a hard tile -- a fill cut short, a band staged in the LDS,
    the tiles one wave holds -- leaks into the frames next to it.  (192, 288) runs the band kernel, (70, 8192) the tile-per-wave one."""
    imgs, _ = R.case_independence(H, W)
    forms, refs = _check_exact(ctx, imgs)
    assert [bool(hard) for _, hard in refs] == [False, False, True, False, False]
    for f in range(len(imgs)):
        alone = _forms(ctx, imgs[f:f + 1])
        for name, got in forms.items():
            assert np.array_equal(got[f], alone[name][0]), (name, f, _where(got[f], alone[name][0]))


def test_near_cap_noise_sandwich(ctx):
    """Three 1080p frames of density-0.38 noise, where natural tiles come closest to the cap (65...95 iterations turn up).  Whatever the
    cap is exactly: the result lies between the filter with no cap and the input, differs from the former only inside tiles the
    reference cannot vouch for, and there keeps or erases whole components."""
    from scipy import ndimage
    imgs = R.case_near_cap()
    forms = _forms(ctx, imgs)
    got = forms["bits"]
    for name, other in forms.items():
        assert np.array_equal(other, got), (name, [_where(a, b) for a, b in zip(other, got)])
    open_tiles = fills = 0
    H, W = imgs.shape[1:]
    for f, img in enumerate(imgs):
        counts, stages = {}, []
        want, hard, unsure = R.despeckle(img, counts=counts, stages=stages)
        full = R.despeckle(img, cap=None)[0]
        assert not (full & ~got[f]).any() and not (got[f] & ~img).any(), f
        allowed = np.zeros((H, W), bool)
        doubtful = sorted(set(hard) | set(unsure))
        for p, y0, x0 in doubtful:
            allowed[max(y0, 0):y0 + 64, max(x0, 0):x0 + 64] = True
        assert not ((got[f] != full) & ~allowed).any(), (f, _where(got[f] & ~allowed, full & ~allowed))
        if not doubtful:
            assert np.array_equal(got[f], want), f
        first_pass_open = [(y0, x0) for p, y0, x0 in doubtful if p == 0]
        for p, y0, x0 in doubtful:
            if p == 1 and any(abs(y0 - y) < 64 and abs(x0 - x) < 64 for y, x in first_pass_open):
                continue                                                     # its input is not known for sure
            box = (slice(max(y0, 0), y0 + 64), slice(max(x0, 0), x0 + 64))
            lab, ncomp = ndimage.label((img if p == 0 else stages[0])[box], structure=np.ones((3, 3)))
            kept = np.unique(lab[got[f][box]])
            gone = np.unique(lab[(lab > 0) & ~got[f][box]])
            assert len(np.intersect1d(kept[kept > 0], gone)) == 0, (f, p, y0, x0)
        open_tiles += len(doubtful)
        fills += len(counts)
    assert open_tiles <= 0.02 * fills, f"{open_tiles} of {fills} tile fills ({100.0 * open_tiles / fills:.2f} %) are hard or unsure"
    # the claim on these frames, with an outline laid over the noise
    framed = imgs[:2] | R.rectangle_outline(H, W, 131, 986, 195, 1603, thick=5)[None]
    _check_search(ctx, framed, _forms(ctx, framed, byte_forms=False)["bits"])
