"""GPU: k_softmax_topk (csrc/k3_cnn.hip) through Context.softmax_topk against a float64 softmax followed by a stable descending sort
(equal probabilities: lowest class first), for every k from 1 to 10 and batches of 1, 255, 256, 257 and 81 * 7 + 5 rows (one thread
per row in 256-thread blocks).  The rows: random at sigma 0.01, 1, 6 and 40; bit-equal logits (all ten, pairs, several at the maximum);
saturated rows (gap > 104: the tail underflows to exactly 0.0, ties at zero, a top-1 of exactly 1.0); finite logits near +-3e38;
-inf among finite values; and, in a test of their own, rows that are not finite (one NaN, all NaN, one +inf, all -inf).

Probabilities, per launch, two bounds, both asserted:
  absolute   |gpu - f64| <= C_ABS * max|torch CPU f32 softmax - f64| + 2^-24 * max|f64|          (cnn_oracle.tolerance as it stands)
  relative   |gpu / f64 - 1| <= C_REL * max|torch CPU f32 softmax / f64 - 1| + 2^-24, plus 2^-126 absolute (an f32 result below the
             smallest normal may be flushed), the same rule on the error relative to the reference probability; the maxima over the
             probabilities of at least 2^-100, below which only the absolute bound applies.
The relative bound is the one that says something about a tail of 1e-9 beside a top-1 of 1, and it is what keeps the index comparison
sharp: rank r must equal the reference's wherever the reference's probabilities at ranks r-1, r and r, r+1 differ by more than twice
the smaller of the two bounds at rank r.  With the absolute bound alone that rule would leave out a quarter of the ranks of the
sigma = 6 rows (their tails lie closer together than 1e-6); test_gap_rule_leaves_out_little holds it to 1 % of the sigma 1 and 6 rows,
on the reference alone.  Among bit-equal logits, and among bit-equal returned probabilities, the lower class comes first,
unconditionally.

C_ABS and C_REL: about four times the largest ratio measured on an MI355X over this file (profiles/softmax_topk_accuracy.txt):
max|gpu - f64| / noise 1.00 at the most, max|gpu / f64 - 1| / relative noise 1.00 at the most
(0.62 for the one-row batch; the largest errors are the same in the kernel and in torch, presumably the f32 rounding of logit - max
that they share), so both are 4."""
import numpy as np
import pytest
import torch

import cnn_oracle

C_ABS = 4.0
C_REL = 4.0
SIZES = [1, 255, 256, 257, 81 * 7 + 5]
SIGMAS = (0.01, 1.0, 6.0, 40.0)
SEED = 7
REL_FROM = 2.0 ** -100
TINY = 2.0 ** -126
_RATIOS = {"abs": 0.0, "rel": 0.0}


def pool():
    """logits f32 [81 * 7 + 5, 10], all rows finite in their results, and the sigma of each random row (0 for a crafted one).  Row 0
    is random; the crafted rows sit at 1..: every batch of 255 or more has them all."""
    rs = np.random.RandomState(SEED)
    n = SIZES[-1]
    sigma = np.array([SIGMAS[i % 4] for i in range(n)])
    z = (rs.randn(n, 10) * sigma[:, None]).astype(np.float32)
    crafted = []
    for v in (0.0, -7.25, 3.0e38, -3.0e38):
        crafted.append(np.full(10, v))                                          # all ten equal
    for _ in range(8):                                                              # pairs equal, anywhere in the order
        row = rs.randn(10) * 2
        a, b, c, d = rs.permutation(10)[:4]
        row[b], row[d] = row[a], row[c]
        crafted.append(row)
    for count in (2, 3, 5):                                                         # several at the maximum
        row = rs.randn(10)
        row[rs.permutation(10)[:count]] = row.max() + 1.5
        crafted.append(row)
    for gap in (104.5, 120.0, 1000.0, 3.0e38):                                      # saturated: the tail is exactly 0.0
        row = rs.randn(10)
        row[rs.randint(0, 10)] += gap + 8
        crafted.append(row)
    row = rs.randn(10) * 3                                                          # saturated with two at the top: 0.5, 0.5, zeros
    row[[2, 6]] = 200.0
    crafted.append(row)
    big = np.float32(3.0e38)
    crafted.append([big, -big, big, 0, 1, -1, np.nextafter(big, np.float32(0)), -big, 2.9e38, -2.9e38])      # max - min overflows f32
    crafted.append(-big + np.arange(10, dtype=np.float32) * np.float32(2.0 ** 104))    # neighbours one ulp of 3e38 apart
    crafted.append(big - np.float32(2.0 ** 104) * (np.arange(10) % 3).astype(np.float32))
    for where in ([0], [9], [1, 2, 3], list(range(1, 10))):                         # -inf among finite values
        row = rs.randn(10) * 2
        row[where] = -np.inf
        crafted.append(row)
    crafted = np.array(crafted, np.float32)
    z[1:1 + len(crafted)] = crafted
    sigma[1:1 + len(crafted)] = 0
    assert 1 + len(crafted) < 255
    return z, sigma


_REF = {}


def reference():
    """The pool, and for it: the float64 softmax [n,10], its stable descending order [n,10], torch's CPU f32 softmax [n,10]."""
    if not _REF:
        z, sigma = pool()
        z64 = z.astype(np.float64)
        with np.errstate(over="ignore"):
            e = np.exp(z64 - z64.max(1, keepdims=True))
        p = e / e.sum(1, keepdims=True)
        order = np.argsort(-p, axis=1, kind="stable")
        _REF.update(z=z, sigma=sigma, p=p, order=order, t=torch.softmax(torch.from_numpy(z.copy()), 1).numpy().astype(np.float64))
        for v in _REF.values():
            v.setflags(write=False)
    return _REF


def bounds(p, t, c_abs=None, c_rel=None):
    """For the rows of one launch: (absolute noise, relative noise, the bound on |gpu - f64| per element [B,10])."""
    c_abs, c_rel = C_ABS if c_abs is None else c_abs, C_REL if c_rel is None else c_rel
    noise = np.abs(t - p).max()
    big = p >= REL_FROM
    rel_noise = (np.abs(t - p)[big] / p[big]).max()
    absolute = cnn_oracle.tolerance(p, noise, c_abs)
    relative = np.where(big, (c_rel * rel_noise + 2.0 ** -24) * p + TINY, np.inf)
    return noise, rel_noise, np.minimum(absolute, relative)


def checked_ranks(P, tol):
    """Which (row, rank) the index comparison covers: the sorted reference probabilities P [B,10] on both sides of the rank are more
    than twice the bound at that rank (tol [B,10], in the same order) away."""
    clear = P[:, :-1] - P[:, 1:] > 2 * np.maximum(tol[:, :-1], tol[:, 1:])
    return np.concatenate([clear[:, :1], clear[:, 1:] & clear[:, :-1], clear[:, -1:]], 1)


def test_gap_rule_leaves_out_little():
    """On the reference alone: of the (row, rank) pairs of the random sigma 1 and sigma 6 rows, the gap rule leaves out at most 1 %,
    in every batch size; and the crafted rows are what the docstring says they are."""
    r = reference()
    for B in SIZES[1:]:
        p, t, order = r["p"][:B], r["t"][:B], r["order"][:B]
        P = np.take_along_axis(p, order, 1)
        covered = checked_ranks(P, np.take_along_axis(bounds(p, t)[2], order, 1))
        rows = np.isin(r["sigma"][:B], (1.0, 6.0))
        assert rows.sum() >= 100 and 1 - covered[rows].mean() <= 0.01, (B, 1 - covered[rows].mean())
    z, p = r["z"], r["p"]
    assert np.isfinite(p).all() and np.abs(p.sum(1) - 1).max() < 1e-12
    p32 = p.astype(np.float32)
    assert ((p32 == 1).sum(1) == 1).sum() >= 4 and ((p32 == 0).sum(1) == 9).sum() >= 4 and ((p32 == 0.5).sum(1) == 2).any()
    assert (np.abs(z) > 2.8e38).any(1).sum() >= 5 and np.isinf(z).any(1).sum() == 4 and not np.isnan(z).any()
    equal = [len(set(row.tolist())) for row in z]
    assert equal.count(1) >= 4 and sum(e in (8, 9) for e in equal) >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("B", SIZES)
def test_softmax_topk_against_float64(ctx, B):
    r = reference()
    z, p, t, order = r["z"][:B], r["p"][:B], r["t"][:B], r["order"][:B]
    noise, rel_noise, tol = bounds(p, t)
    P, T = np.take_along_axis(p, order, 1), np.take_along_axis(tol, order, 1)
    covered = checked_ranks(P, T)
    dz = torch.from_numpy(z.copy()).to(ctx.device)
    for k in range(1, 11):
        idx, prob = ctx.softmax_topk(dz, k)
        assert idx.shape == (B, k) and prob.shape == (B, k) and idx.dtype == torch.uint8 and prob.dtype == torch.float32
        idx, prob = idx.cpu().numpy().astype(np.int64), prob.cpu().numpy()
        assert np.isfinite(prob).all() and (prob >= 0).all() and (idx < 10).all()
        assert (np.sort(idx, 1)[:, 1:] != np.sort(idx, 1)[:, :-1]).all(), "an index repeats"
        assert (prob[:, 1:] <= prob[:, :-1]).all(), "probabilities increase"
        got = prob.astype(np.float64)
        mine = np.take_along_axis(p, idx, 1)                               # the reference probability of the class the kernel names
        err = np.maximum(np.abs(got - P[:, :k]), np.abs(got - mine))
        big = P[:, :k] >= REL_FROM
        _RATIOS["abs"] = max(_RATIOS["abs"], err.max() / noise)
        big &= mine >= REL_FROM
        _RATIOS["rel"] = max(_RATIOS["rel"], (err[big] / np.minimum(P[:, :k], mine)[big]).max() / rel_noise)
        print(f"B {B} k {k}: max|gpu - f64| {err.max():.3e} noise {noise:.3e} ratio {err.max() / noise:.2f}; relative noise {rel_noise:.3e} "
              f"largest ratios so far: absolute {_RATIOS['abs']:.2f} relative {_RATIOS['rel']:.2f}")
        assert (np.abs(got - P[:, :k]) <= T[:, :k]).all() and (np.abs(got - mine) <= np.take_along_axis(tol, idx, 1)).all()
        assert (idx == order[:, :k])[covered[:, :k]].all()
        # ties: bit-equal logits, and bit-equal results, come lowest class first
        for a in range(k - 1):
            same_logit = np.take_along_axis(z, idx[:, a:a + 1], 1) == np.take_along_axis(z, idx[:, a + 1:], 1)
            assert (idx[:, a:a + 1] < idx[:, a + 1:])[same_logit].all()
            tie = prob[:, a] == prob[:, a + 1]
            assert (idx[tie, a] < idx[tie, a + 1]).all()
        top2 = np.sort(z.astype(np.float64), 1)[:, -2:]
        sat = top2[:, 1] - top2[:, 0] > 104                                 # every other exp underflows: exactly 1.0, then ties at 0.0
        assert (prob[sat, 0] == 1).all() and (prob[sat, 1:] == 0).all() and (sat.sum() >= 4 or B == 1)


def bad_rows():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    base = np.array([0.5, -1, 2, 0, 3, -2, 1, 4, -3, 0.25], np.float32)
    rows = []
    for j in (0, 4, 9):
        row = base.copy()
        row[j] = nan
        rows.append(row)
    rows.append(np.full(10, nan))
    for j in (0, 7):
        row = base.copy()
        row[j] = inf
        rows.append(row)
    rows.append(np.full(10, -inf))
    return np.array(rows, np.float32)


@pytest.mark.gpu
def test_rows_that_are_not_finite(ctx):
    """One NaN, all NaN, one +inf, all -inf: every probability of the row is NaN, its k indices are still distinct, and the other rows
    of the launch are bit-identical to a launch without the bad rows (at the start, across the 256-thread block boundary, at the end)."""
    good = reference()["z"][:300].copy()
    bad = bad_rows()
    at = [0, 100, 254, 255, 256, 257, 306]
    mixed = np.insert(good, [0, 99, 252, 252, 252, 252, 300], bad, axis=0)
    assert mixed.shape[0] == 307 and all(np.array_equal(mixed[a], bad[i], equal_nan=True) for i, a in enumerate(at))
    keep = np.setdiff1d(np.arange(307), at)
    for k in range(1, 11):
        gi, gp = [v.cpu().numpy() for v in ctx.softmax_topk(torch.from_numpy(good).to(ctx.device), k)]
        mi, mp = [v.cpu().numpy() for v in ctx.softmax_topk(torch.from_numpy(mixed).to(ctx.device), k)]
        assert mi[keep].tobytes() == gi.tobytes() and mp[keep].tobytes() == gp.tobytes()
        assert np.isnan(mp[at]).all() and (mi[at] < 10).all()
        assert (np.sort(mi[at], 1)[:, 1:] != np.sort(mi[at], 1)[:, :-1]).all(), mi[at].tolist()
        if k == 10:
            assert (np.sort(mi[at], 1) == np.arange(10)).all()
