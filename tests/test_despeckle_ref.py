"""The speck filter's reference (tests/despeckle_ref.py) against itself, and the table of inputs tests/test_gpu_despeckle_topology.py
feeds the kernels: every placed tile is in the regime it is named for, and the inputs of the exact comparisons have no tile whose fate
depends on the details of the fill schedule.  No GPU."""
import numpy as np
import pytest

import despeckle_ref as R


def _builders():
    out = {}
    for how in R.ORIENTATIONS:
        for nd in (2, 4, 8):
            out[f"boustrophedon {nd} {how}"] = R.boustrophedon(nd, how=how)
        out[f"boustrophedon low box {how}"] = R.boustrophedon(8, rows=(2, 35), how=how)
        out[f"boustrophedon cut {how}"] = R.boustrophedon(2, 66, how=how)
        for kind in ("capped", "long", "spiral", "easy"):
            out[f"{kind} {how}"] = R.special(kind, how)
        out[f"spiral 2 {how}"] = R.spiral(2, how)
    for seed in R.LONG_NOISE_SEEDS:
        out[f"noise {seed}"] = R.noise(0.38, seed)
    return out


def test_fixed_point_is_the_labelling():
    """fill_iterations asserts that the schedule's fixed point is tile_keep; run it on random tiles at densities 0.2 ... 0.55 (either side of
    the percolation threshold) and on every builder's output.  tile_keep itself against a breadth-first search on some of them."""
    rs = np.random.RandomState(1)
    worst = 0
    for k in range(320):
        worst = max(worst, R.fill_iterations(rs.uniform(size=(64, 64)) < 0.2 + 0.05 * (k % 8)))
    assert 40 <= worst < 96, worst                                       # the regime the issue's model saw: deep, but settling
    tiles = _builders()
    for name, tile in tiles.items():
        R.fill_iterations(tile)
    for tile in [rs.uniform(size=(64, 64)) < 0.4, rs.uniform(size=(40, 64)) < 0.4, tiles["capped t"], tiles["spiral lr"][:, :50]]:
        for sides in ((True, True, True, True), (False, True, True, False), (True, False, False, True)):
            seen = np.zeros(tile.shape, bool)
            h, w = tile.shape
            stack = [(y, x) for y in range(h) for x in range(w)
                     if tile[y, x] and ((sides[0] and y == 0) or (sides[1] and y == h - 1) or (sides[2] and x == 0) or (sides[3] and x == w - 1))]
            for y, x in stack:
                seen[y, x] = True
            while stack:
                y, x = stack.pop()
                for yy in range(max(y - 1, 0), min(y + 2, h)):
                    for xx in range(max(x - 1, 0), min(x + 2, w)):
                        if tile[yy, xx] and not seen[yy, xx]:
                            seen[yy, xx] = True
                            stack.append((yy, xx))
            assert np.array_equal(seen, R.tile_keep(tile, sides))


def test_builder_regimes():
    """The counts the tiles are built for, in all four orientations: a 1-pixel diagonal path costs about an iteration per pixel."""
    for how in R.ORIENTATIONS:
        assert R.fill_iterations(R.special("capped", how)) >= 300
        assert R.fill_iterations(R.boustrophedon(8, rows=(2, 35), how=how)) >= 150
        assert R.fill_iterations(R.boustrophedon(8, rows=(2, 35), cols=(2, 29), how=how)) >= 150
        assert 50 <= R.fill_iterations(R.special("long", how)) <= 64
        assert 50 <= R.fill_iterations(R.special("long", how, rows=(2, 35))) <= 64
        assert 50 <= R.fill_iterations(R.special("spiral", how)) <= 64
        assert R.fill_iterations(R.special("easy", how)) <= 4
        assert R.fill_iterations(R.spiral(2, how)) <= 64
    for seed in R.LONG_NOISE_SEEDS:
        tile = R.noise(0.38, seed)
        assert 50 <= R.fill_iterations(tile) <= 64
        assert not np.array_equal(tile, tile.T) and not np.array_equal(tile, tile[:, ::-1])
    # the path is one component, and mirrored / transposed tiles are what they say
    from scipy import ndimage
    tile = R.boustrophedon(8)
    assert ndimage.label(tile, structure=np.ones((3, 3)))[1] == 1
    assert np.array_equal(R.boustrophedon(8, how="lr"), tile[:, ::-1]) and np.array_equal(R.boustrophedon(8, how="t"), tile.T)
    img = R.place(np.zeros((100, 100), bool), 10, 20, tile)
    assert np.array_equal(img[10:74, 20:84], tile) and img.sum() == tile.sum()


def _cases():
    odd = R.case_bytes_odd()
    return {"topology": R.case_topology(), "strip": R.case_strip(), "odd 130x250": odd[0], "odd 67x61": odd[1], "words 200x96": R.case_words(200, 96),
            "words 1080p": R.case_words(1080, 1920), "independence 192x288": R.case_independence(192, 288),
            "independence strip": R.case_independence(70, 8192)}


@pytest.mark.parametrize("name", ["topology", "strip", "odd 130x250", "odd 67x61", "words 200x96", "words 1080p", "independence 192x288",
                                  "independence strip"])
def test_input_table(name):
    """Every placed tile of every exact-comparison input is in its regime in the pass it targets -- easy <= 64, long 50...64, capped >= 150
    iterations -- and no tile of either pass is unsure.  Frames with capped tiles have pixels that survive only because of the cap."""
    imgs, tiles = _cases()[name]
    for f, img in enumerate(imgs):
        counts = {}
        want, hard, unsure = R.despeckle(img, counts=counts)
        assert unsure == [], (name, f, unsure)
        placed = [t for t in tiles if t[0] == f]
        for _, regime, p, y0, x0 in placed:
            c = counts[(p, y0, x0)]
            if regime == "capped":
                assert c >= 150 and (p, y0, x0) in hard, (name, f, regime, p, y0, x0, c)
            elif regime == "long":
                assert 50 <= c <= 64, (name, f, regime, p, y0, x0, c)
            else:
                assert c <= 64, (name, f, regime, p, y0, x0, c)
        assert sorted(hard) == sorted((p, y0, x0) for _, regime, p, y0, x0 in placed if regime == "capped"), (name, f)
        assert max(counts.values()) <= 64 or hard, (name, f)
        full = R.despeckle(img, cap=None)[0]
        assert not (full & ~want).any() and not (want & ~img).any()
        if any(regime == "capped" and p == 0 for _, regime, p, _, _ in placed):
            assert (want & ~full).any(), (name, f)                            # a speck that only the cap saved
        assert (img & ~want).any(), (name, f)                                # and something is erased at all
    if name == "topology":
        _, hard, _ = R.despeckle(imgs[0])
        assert {p for p, _, _ in hard} == {0, 1}
        assert {regime for _, regime, _, _, _ in tiles} == {"capped", "long", "easy"}


def test_near_cap_noise():
    """Density-0.38 noise at 1080p is the natural input next to the cap: tiles beyond 64 iterations exist, and the tiles whose fate the
    margins leave open stay under 2 % of the tile fills (the bound the GPU test repeats)."""
    for img in R.case_near_cap()[:1]:
        counts = {}
        want, hard, unsure = R.despeckle(img, counts=counts)
        assert max(counts.values()) > 64
        assert len(hard) + len(unsure) <= 0.02 * len(counts), (len(hard), len(unsure), len(counts))
        assert not (R.despeckle(img, cap=None)[0] & ~want).any()
