"""GPU (-m gpu): MC dropout on DigitCNNv3 (sv_cnn3_forward_mc_f32, csrc/k8_cnn_v3.hip; DigitCNNv3.forward_with_uncertainty) against a
float64 evaluation of the unfolded model with the same keep masks (tests/model_v3_mc_ref.py).

Per-sample logits: the rule of tests/test_gpu_model_v3.py as it is, both references evaluated with the same masks,
        max|gpu - f64| <= C_V3 * max|torch_f32 - f64| + 2^-24 * max|f64|                      (= tol)
mean_probs: |dp| <= p expm1(2 tol / |T|) + 2e-6;  std_probs: |dstd| <= sqrt(S / (S - 1)) e + 2e-6 with e the largest per-sample
probability bound (model_v3_mc_ref.bounds has the argument);  predicted: equal wherever the reference's top-2 gap of mean_probs exceeds
twice its bound, and at most 1 % of the cells may fall under that gap (asserted).
Batches are checked on a fixed subset of cells around the chunk boundaries (SV_V3_SUBBATCH / S cells per chunk): the f64 reference runs
on the CPU.

Measured on an MI355X (profiles/model_v3_mc_accuracy.txt): the largest ratio max|gpu - f64| / noise is 2.87 (S = 2, B = 1 with SE), at most
2.2 over the other shapes, the temperatures and the module drop-in, against C_V3 = 16; mean_probs is within 5.1e-7 and std_probs within
7.2e-7 of float64 everywhere."""
import os
import sys

import numpy as np
import pytest
import torch

import cnn_oracle
import model_v3_mc_ref as mc
import model_v3_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUB = 512                           # SV_V3_SUBBATCH of include/sudoku_vision_hip.h
SEED, OFFSET = 0x1234567887654321, 8
P_SP, P_FC = 0.1, 0.5
SHAPES = ((1, 1), (2, 1), (3, 2), (10, 81), (7, 81), (2, 513))
_X = ref.inputs(5, 513)
_SD = {}


def _sd(use_se, temperature=1.0):
    if (use_se, temperature) not in _SD:
        sd = {k: v.clone() for k, v in ref.random_state_dict_v3(2024, use_se).items()}
        sd["temperature"][:] = temperature
        _SD[use_se, temperature] = sd
    return _SD[use_se, temperature]


def _cells(S, B):
    """The cells checked against float64: all of a small batch, else the first and last, those around every chunk boundary, every 16th."""
    per = SUB // S
    near = [c for b in range(per, B, per) for c in (b - 1, b, b + 1)]
    return np.arange(B) if B * S <= 32 else np.unique(np.clip(np.array([0, 1, B - 2, B - 1] + near + list(range(0, B, 16))), 0, B - 1))


def _mc(ctx, x, S, p_sp=P_SP, p_fc=P_FC, seed=SEED, offset=OFFSET, masks=None, **kw):
    """-> mean, std, predicted (, logits) (, (keep1, keep3, keepf)) as numpy"""
    if masks is not None:
        masks = tuple(torch.from_numpy(np.ascontiguousarray(m)).cuda() for m in masks)
    out = ctx.cnn3_forward_mc(torch.from_numpy(np.ascontiguousarray(x)).cuda(), S, p_sp, p_fc, seed, offset, masks=masks, **kw)
    torch.cuda.synchronize()
    return tuple(tuple(m.cpu().numpy() for m in o) if isinstance(o, tuple) else o.cpu().numpy() for o in out)


def _check(what, sd, x, keep, got, temperature=1.0, p_sp=P_SP, p_fc=P_FC):
    """got = (mean, std, predicted, logits [S,n,10]) of the cells x [n,1,28,28] under keep (three [S,n,C]) against the float64 reference."""
    mean, std, predicted, logits = got
    S, n = logits.shape[:2]
    xe, ke = mc.expand(x, keep)
    want = mc.forward64(sd, xe, ke, p_sp, p_fc).numpy()
    noise = float(np.abs(mc.forward(sd, xe, ke, p_sp, p_fc).numpy().astype(np.float64) - want).max())
    tol = cnn_oracle.tolerance(want, noise, ref.C_V3)
    err = float(np.abs(logits.reshape(-1, 10).astype(np.float64) - want).max()) if np.isfinite(logits).all() else float("inf")
    print(f"ACCMC {what}: err {err:.3e} noise {noise:.3e} ratio {err / max(noise, 1e-300):.3f} tol {tol:.3e}")
    assert err <= tol, (what, err, noise, tol)
    probs64, mean64, std64, pred64 = mc.stats(want.reshape(S, n, 10), temperature)
    mean_bound, std_bound = mc.bounds(probs64, mean64, tol, temperature)
    d_mean = np.abs(mean - mean64)
    print(f"ACCMC {what}: mean err {d_mean.max():.3e} (bound at least {mean_bound.min():.3e})", end="")
    assert (d_mean <= mean_bound).all(), what
    if S > 1:
        d_std = np.abs(std - std64)
        print(f", std err {d_std.max():.3e} (bound {std_bound:.3e})")
        assert (d_std <= std_bound).all(), what
    else:
        print()
        assert np.isnan(std).all(), what
    top2 = np.sort(mean64, 1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 2 * np.sort(mean_bound, 1)[:, -1]
    assert (~clear).sum() <= 0.01 * n, (what, "cells under the top-2 gap", int((~clear).sum()), n)
    assert predicted.dtype == np.int64 and (predicted[clear] == pred64[clear]).all(), what
    return err / max(noise, 1e-300)


@pytest.mark.parametrize("use_se", (True, False))
@pytest.mark.parametrize("S,B", SHAPES)
def test_injected_masks_against_f64(ctx, S, B, use_se):
    """(7, 81): 567 (sample, cell) pairs in chunks of 73 cells, the boundary inside the batch; (2, 513): more cells than SV_V3_SUBBATCH."""
    import sudoku_vision_amd as sva
    sd = _sd(use_se)
    ctx.load_state_dict_v3(sd)
    keep = sva.host.mc_dropout_masks(SEED, OFFSET, S, B, P_SP, P_FC)
    mean, std, predicted, logits = _mc(ctx, _X[:B], S, masks=keep, want_logits=True)
    sel = _cells(S, B)
    _check(f"injected S={S} B={B} se={use_se}", sd, _X[:B][sel], tuple(k[:, sel] for k in keep), (mean[sel], std[sel], predicted[sel], logits[:, sel]))


@pytest.mark.parametrize("S,B", ((7, 81), (1, 1), (2, 513)))
def test_generated_masks_are_the_host_generators(ctx, S, B):
    import sudoku_vision_amd as sva
    ctx.load_state_dict_v3(_sd(True))
    keep = sva.host.mc_dropout_masks(SEED, OFFSET, S, B, P_SP, P_FC)
    injected = _mc(ctx, _X[:B], S, masks=keep, want_logits=True, want_masks=True)
    generated = _mc(ctx, _X[:B], S, want_logits=True, want_masks=True)
    for k in range(3):
        assert np.array_equal(generated[4][k], keep[k]) and np.array_equal(injected[4][k], keep[k])
    for a, b in zip(injected[:4], generated[:4]):
        assert np.array_equal(a, b, equal_nan=True)
    other = _mc(ctx, _X[:B], S, offset=OFFSET + 4, want_masks=True)
    assert not np.array_equal(other[3][2], keep[2])


def test_exact_invariants(ctx):
    sd = _sd(True, 1.7)
    ctx.load_state_dict_v3(sd)
    B, S = 81, 7
    x = _X[:B]
    plain, digits, conf = (o.cpu().numpy() for o in ctx.cnn3_forward(torch.from_numpy(x).cuda(), want_digits=True))
    # both rates 0: every sample is the eval forward
    mean, std, predicted, logits = _mc(ctx, x, S, p_sp=0.0, p_fc=0.0, want_logits=True)
    assert all(np.array_equal(logits[s], plain) for s in range(S))
    assert (std == 0).all()
    assert np.array_equal(predicted, digits.astype(np.int64))
    assert (np.abs(mean[np.arange(B), digits] - conf) <= conf * np.expm1(2 * 2.0 ** -22) + 2e-6).all()      # two f32 softmaxes of equal logits
    # feature keep all zero: the logits are the fc bias
    ones = [np.ones((S, B, c), np.uint8) for c in mc.SITE_CHANNELS]
    mean, std, predicted, logits = _mc(ctx, x, S, masks=(ones[0], ones[1], 0 * ones[2]), want_logits=True)
    assert (logits == sd["fc.bias"].numpy()).all() and (std == 0).all()
    mean, std, predicted, logits = _mc(ctx, x, S, p_fc=1.0, want_logits=True)
    assert (logits == sd["fc.bias"].numpy()).all() and (std == 0).all()
    # one dropped layer1 channel on one sample of one cell changes that sample's logits only
    k1 = ones[0].copy()
    k1[3, 40, 5] = 0
    mean, std, predicted, logits = _mc(ctx, x, S, p_sp=0.0, p_fc=0.0, masks=(k1, ones[1], ones[2]), want_logits=True)
    moved = (logits != plain[None]).any(2)
    assert moved[3, 40] and moved.sum() == 1
    assert (std[np.arange(B) != 40] == 0).all() and (std[40] > 0).any()
    # S = 1: std is NaN, mean is that sample's softmax
    mean, std, predicted, logits = _mc(ctx, x, 1, want_logits=True)
    assert np.isnan(std).all()
    p64 = mc.stats(logits, 1.7)[1]
    assert np.abs(mean - p64).max() <= 2e-6


def test_batch_independence_and_repeatability(ctx):
    import sudoku_vision_amd as sva
    ctx.load_state_dict_v3(_sd(True))
    S, B = 7, 81
    keep = sva.host.mc_dropout_masks(SEED, OFFSET, S, B, P_SP, P_FC)
    big = _mc(ctx, _X[:B], S, want_logits=True)
    again = _mc(ctx, _X[:B], S, want_logits=True)
    for a, b in zip(big, again):
        assert np.array_equal(a, b)
    for i in (0, 72, 73, 80):                                       # alone, with the masks of its cell index
        one = _mc(ctx, _X[i:i + 1], S, masks=tuple(k[:, i:i + 1] for k in keep), want_logits=True)
        assert all(np.array_equal(o[..., 0, :] if o.ndim == 3 else o[0], g[..., i, :] if g.ndim == 3 else g[i]) for o, g in zip(one, big)), i
    y = _X[:B].copy()
    y[40, 0, 3, 3] = np.nan                                         # a NaN cell does not disturb its neighbours
    got = _mc(ctx, y, S, want_logits=True)
    ok = np.arange(B) != 40
    assert np.array_equal(got[0][ok], big[0][ok]) and np.array_equal(got[1][ok], big[1][ok]) and np.array_equal(got[3][:, ok], big[3][:, ok])


@pytest.mark.parametrize("temperature", (0.5, 3.0))
def test_temperature(ctx, temperature):
    import sudoku_vision_amd as sva
    sd = _sd(True, temperature)
    ctx.load_state_dict_v3(sd)
    S, B = 5, 16
    keep = sva.host.mc_dropout_masks(SEED, OFFSET, S, B, P_SP, P_FC)
    got = _mc(ctx, _X[:B], S, want_logits=True)
    _check(f"temperature {temperature}", sd, _X[:B], keep, got, temperature=temperature)
    cold = mc.stats(got[3], 1.0)[1]
    assert np.abs(cold - got[0]).max() > 1e-2                       # the temperature is in there


def _dropin():
    sys.path.insert(0, os.path.join(ROOT, "sudoku-vision_amd", "ml"))
    try:
        import model_v3
    finally:
        sys.path.pop(0)
    return model_v3


def test_module_dropin(ctx):
    import sudoku_vision_amd as sva
    model_v3 = _dropin()
    sd = _sd(True, 1.3)
    m = model_v3.DigitCNNv3()
    m.load_state_dict({**{k: v for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")}, **sd}, strict=True)
    m = m.cuda().eval()
    B = 33
    xd = torch.from_numpy(_X[:B]).cuda()
    before = m(xd).clone()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    torch.manual_seed(5)
    gen = torch.cuda.default_generators[xd.device.index]
    seed, offset = gen.initial_seed(), gen.get_offset()
    a = m.forward_with_uncertainty(xd)
    assert not m.training and gen.get_offset() == offset + 4
    b = m.forward_with_uncertainty(xd)                               # no reseeding: other masks
    torch.manual_seed(5)
    m.train()                                                       # the reference's callers may leave it so; accepted here and only here
    c = m.forward_with_uncertainty(xd, n_samples=10)
    assert not m.training
    assert all(torch.equal(p, q) for p, q in zip(a, c)) and not torch.equal(a[0], b[0])
    assert a[0].shape == (B, 10) and a[1].shape == (B, 10) and a[2].shape == (B,) and a[2].dtype == torch.int64 and a[0].is_cuda
    # what the module computed is the context's entry at the generator's seed and offset, within the float64 bounds
    keep = sva.host.mc_dropout_masks(seed, offset, 10, B, m.spatial_dropout.p, m.dropout.p)
    direct = sva.default_context(xd.device).cnn3_forward_mc(xd, 10, 0.1, 0.5, seed, offset, want_logits=True)
    assert all(torch.equal(p, q) for p, q in zip(a, direct[:3]))
    sel = np.arange(0, B, 4)
    _check("module", sd, _X[:B][sel], tuple(k[:, sel] for k in keep), tuple(t.cpu().numpy()[..., sel, :] if t.dim() > 1 else t.cpu().numpy()[sel] for t in direct), temperature=1.3)
    own = torch.Generator(device=xd.device)
    own.manual_seed(77)
    d = m.forward_with_uncertainty(xd, 4, generator=own)
    assert own.get_offset() == 4 and gen.get_offset() == offset + 4
    assert torch.equal(d[0], sva.default_context(xd.device).cnn3_forward_mc(xd, 4, 0.1, 0.5, 77, 0)[0])
    # weights and running statistics are untouched: a later forward is the earlier one
    assert all(torch.equal(v, state[k]) for k, v in m.state_dict().items())
    assert torch.equal(m(xd), before)
    m.dropout.p = 0.0
    m.spatial_dropout.p = 0.0
    mean, std, _ = m.forward_with_uncertainty(xd, 3)
    assert (std == 0).all()
    with pytest.raises(ValueError):
        m.forward_with_uncertainty(xd, 0)


def test_side_stream_and_graph_replay():
    """The entry on a busy side stream (a delay, then the input copied in behind it, then the call: the result is the late input's), and
    captured into a graph after reserve (capture_error_mode "global": an allocation or a synchronisation by the library raises)."""
    import sudoku_vision_amd as sva
    c = sva.Context()
    c.load_state_dict_v3(_sd(True))
    c.reserve(81)
    S, B = 7, 81
    A, Bx = torch.from_numpy(_X[:B]).cuda(), torch.from_numpy(_X[100:100 + B]).cuda()
    call = lambda x: c.cnn3_forward_mc(x, S, P_SP, P_FC, SEED, OFFSET, want_logits=True)
    want_a, want_b = [t.clone() for t in call(A)], [t.clone() for t in call(Bx)]
    buf = A.clone()
    torch.cuda.synchronize()
    assert not torch.equal(want_a[0], want_b[0])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(20_000_000)
        buf.copy_(Bx, non_blocking=True)
        late = call(buf)
    s.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(late, want_b))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="global"):
        out = call(buf)
    for x, want in ((A, want_a), (Bx, want_b), (Bx, want_b)):
        buf.copy_(x)
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(p, q) for p, q in zip(out, want))        # the captured seed, offset and masks repeat
    c.close()


def test_error_paths():
    import ctypes as C
    import sudoku_vision_amd as sva
    from sudoku_vision_amd._native import NativeError
    c = sva.Context()
    x = torch.zeros(2, 1, 28, 28, device="cuda")
    with pytest.raises(NativeError, match="SV_ERR_NO_WEIGHTS"):
        c.cnn3_forward_mc(x, 3, 0.1, 0.5, 1, 0)
    c.load_state_dict_v3(_sd(False))
    c.set_precision(c.PREC_BF16)
    with pytest.raises(NativeError, match="SV_ERR_UNSUPPORTED"):
        c.cnn3_forward_mc(x, 3, 0.1, 0.5, 1, 0)
    c.set_precision(c.PREC_F32)
    for S, p_sp, p_fc in ((0, 0.1, 0.5), (3, 1.0, 0.5), (3, -0.1, 0.5), (3, 0.1, 1.5), (3, float("nan"), 0.5)):
        with pytest.raises(ValueError):
            c.cnn3_forward_mc(x, S, p_sp, p_fc, 1, 0)
    lib, null = sva._native.lib(), None
    raw = lambda S, p_sp, p_fc, B=2, k1=None: lib.sv_cnn3_forward_mc_f32(c._h, C.c_void_p(x.data_ptr()), B, S, p_sp, p_fc, 1, 0, k1, null, null, null, null, null, null,
                                                                          null, null, null, None)
    assert [raw(0, 0.1, 0.5), raw(SUB + 1, 0.1, 0.5), raw(3, 1.0, 0.5), raw(3, 0.1, 1.5), raw(3, float("nan"), 0.5), raw(3, 0.1, 0.5, B=-1)] == [-1] * 6
    assert raw(3, 0.1, 0.5, k1=C.c_void_p(x.data_ptr())) == -1        # one mask of three
    assert raw(3, 0.1, 0.5, B=0) == 0 and raw(SUB, 0.1, 1.0) == 0      # every output NULL
    torch.cuda.synchronize()
    mean, std, pred = c.cnn3_forward_mc(x, 2, 0.1, 0.5, 1, 0)
    assert mean.shape == (2, 10) and std.shape == (2, 10) and pred.shape == (2,)
    c.close()
