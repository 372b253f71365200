"""CPU: tests/jpeg_encode_ref.py, the restatement the encoder's GPU and host tests use as their oracle, writes Pillow's (libjpeg-turbo's)
file byte for byte -- every size, sampling, quality and restart interval of the case list, on every kind of content."""
import numpy as np
import pytest

import jpeg_encode_ref as R


@pytest.mark.parametrize("kind", R.CONTENTS)
@pytest.mark.parametrize("sampling", list(R.SAMPLINGS))
def test_restatement_equals_pillow(sampling, kind):
    """noise: long codes and large magnitude categories; checker / zeros / ones: extremes, DC-only and EOB-only blocks; ramp: runs of 16 and more
    zeros (ZRL); photo: a crop of tests/golden/sample_1.jpg.  8x8 and 1x1 at 4:2:0 have dummy blocks, 17x33 both edge replications."""
    sizes = R.SIZES + ([(64, 64)] if kind == "photo" else [])
    for H, W in sizes:
        img = R.content(kind, H, W, sampling == "gray")
        for q in R.QUALITIES:
            for restart in R.RESTARTS:
                assert R.encode(img, q, sampling, restart) == R.pillow_encode(img, q, sampling, restart), (H, W, q, restart)


def test_the_case_list_reaches_what_it_names():
    """ZRL in the ramp, magnitude category 10 in the noise, dummy blocks at 4:2:0, and a quantiser input exactly half way between two steps."""
    for q in (75, 95, 100):
        geo, coef, _ = R.forward(R.content("ramp", 40, 24), q, "444")
        longest = 0
        for row in coef.reshape(-1, 64)[:, R.NATURAL]:
            nz = np.flatnonzero(row)
            if nz.size > 1:
                longest = max(longest, np.diff(nz).max() - 1)
        assert longest >= 16, q
    _, coef, _ = R.forward(R.content("checker", 16, 16), 100, "444")
    assert np.abs(coef.reshape(-1, 64)[:, 1:]).max() >= 512
    for H, W in ((8, 8), (1, 1)):
        geo = R.Geometry(W, H, "420")
        assert geo.own_bw[0] < geo.bw[0] and geo.own_bh[0] < geo.bh[0]
    geo = R.Geometry(33, 17, "420")
    assert geo.own_bw[0] * 8 > 33 and geo.own_bh[0] * 8 > 17 and geo.own_bw[1] * 16 > 33 and geo.own_bh[1] * 16 > 17


def test_sparse_form_is_the_decoders():
    """masks over zigzag positions, offsets = exclusive prefix sums of the popcounts, values in zigzag order"""
    _, coef, _ = R.forward(R.content("noise", 17, 33), 75, "420")
    masks, offsets, values = R.sparse(coef)
    zz = coef.reshape(-1, 64)[:, R.NATURAL]
    at = 0
    for b in range(zz.shape[0]):
        assert offsets[b] == at
        for k in range(64):
            assert bool(int(masks[b]) >> k & 1) == (zz[b, k] != 0)
            if zz[b, k]:
                assert values[at] == zz[b, k]
                at += 1
    assert at == values.size
