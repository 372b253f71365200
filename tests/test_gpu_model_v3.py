"""GPU (-m gpu): the DigitCNNv3 forward (csrc/k8_cnn_v3.hip) through the C ABI via Context, against a float64 evaluation of the unfolded
model (tests/model_v3_ref.py).

Tolerance rule (scale-free; per batch, over the cells checked), for logits and for features:
        max|gpu - f64| <= C_V3 * max|torch_f32 - f64| + 2^-24 * max|f64|
The noise term is the error of PyTorch-CPU's own f32 evaluation of the same unfolded model against float64.  Digits must be equal wherever
the reference's top-2 gap exceeds twice the tolerance (at most 1 % of a batch's cells may fall under that gap: asserted); conf
(softmax(logits / temperature) at the argmax) within the tolerance carried through the softmax.
Large batches are checked on a fixed subset (first 513 and last 128 cells and every k-th): the f64 reference runs on the CPU.

C_V3 = 16 (model_v3_ref): about four times the largest ratio max|gpu - f64| / noise measured on an MI355X over this file.
Measured ratios (profiles/r06_model_v3_accuracy.txt): 3.68 at the most (logits of the one-cell batch without SE), 3.62 for the features with
every layer scaled by 1e-3 (almost all BatchNorm bias there), at most 2.8 over the other batch sizes, 8-bit cells with either glue, the other
hard weight sets, the module drop-in and recognize_image."""
import os
import sys

import numpy as np
import pytest
import torch

import cnn_oracle
import model_v3_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUB = 512                           # SV_V3_SUBBATCH of include/sudoku_vision_hip.h
BIG = 81 * 64 + 1
SIZES = [1, 2, 3, 15, 16, 17, 63, 64, 65, 81, SUB - 1, SUB, SUB + 1, BIG]
CHECKED = np.unique(np.concatenate([np.arange(SUB + 1), np.arange(BIG - 128, BIG), np.arange(0, BIG, 40)]))
_POOL = {}


def _pool(use_se):
    """One pool of BIG f32 cells per model variant, with the f64 / f32 references of the cells in CHECKED computed once."""
    if use_se not in _POOL:
        sd = ref.random_state_dict_v3(2024, use_se)
        x = ref.inputs(5, BIG)
        lg64, ft64 = ref.forward64(sd, x[CHECKED], return_features=True)
        lg32, ft32 = ref.forward(sd, x[CHECKED], return_features=True)
        _POOL[use_se] = (sd, x, lg64.numpy(), ft64.numpy(), lg32.numpy().astype(np.float64), ft32.numpy().astype(np.float64))
    return _POOL[use_se]


def _check(what, logits, want, want32, digits=None, conf=None, temperature=1.0):
    noise = float(np.abs(want32 - want).max())
    tol = cnn_oracle.tolerance(want, noise, ref.C_V3)
    err = float(np.abs(logits.astype(np.float64) - want).max()) if np.isfinite(logits).all() else float("inf")
    print(f"ACC3 {what}: err {err:.3e} noise {noise:.3e} ratio {err / max(noise, 1e-300):.3f} tol {tol:.3e}")
    assert err <= tol, (what, err, noise, tol)
    if digits is not None:
        top2 = np.sort(want, 1)[:, -2:]
        clear = top2[:, 1] - top2[:, 0] > 2 * tol
        assert (~clear).sum() <= 0.01 * len(want), (what, "cells under the top-2 gap", int((~clear).sum()), len(want))
        assert (digits[clear] == want.argmax(1)[clear]).all(), what
        z = want / temperature
        arg = want.argmax(1)
        conf_want = 1.0 / np.exp(z - z[np.arange(len(z)), arg][:, None]).sum(1)
        t = min(2 * tol / abs(temperature), 50.0)
        assert (np.abs(conf[clear] - conf_want[clear]) <= conf_want[clear] * np.expm1(t) + 2e-6).all(), what
    return err / max(noise, 1e-300)


def _refs(sd, x):
    lg64, ft64 = ref.forward64(sd, x, return_features=True)
    lg32, ft32 = ref.forward(sd, x, return_features=True)
    return lg64.numpy(), ft64.numpy(), lg32.numpy().astype(np.float64), ft32.numpy().astype(np.float64)


def _run(ctx, x, **kw):
    out = ctx.cnn3_forward(torch.from_numpy(x).cuda(), **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out) if isinstance(out, tuple) else out.cpu().numpy()


@pytest.mark.parametrize("use_se", (True, False))
@pytest.mark.parametrize("B", SIZES)
def test_f32_over_batch_sizes(ctx, B, use_se):
    sd, x, lg64, ft64, lg32, ft32 = _pool(use_se)
    ctx.load_state_dict_v3(sd)
    logits, digits, conf, feats = _run(ctx, x[:B], want_digits=True, want_features=True)
    sel = CHECKED[CHECKED < B] if B < BIG else CHECKED
    k = np.searchsorted(CHECKED, sel)
    _check(f"f32 B={B} se={use_se} logits", logits[sel], lg64[k], lg32[k], digits[sel], conf[sel])
    _check(f"f32 B={B} se={use_se} features", feats[sel], ft64[k], ft32[k])


@pytest.mark.parametrize("use_se", (True, False))
@pytest.mark.parametrize("glue", (0, 1))
@pytest.mark.parametrize("B", (81, SUB + 1))
def test_u8_cells(ctx, B, glue, use_se):
    rs = np.random.RandomState(B + glue)
    cells = rs.randint(0, 256, (B, 28, 28)).astype(np.uint8)
    cells[::3] = np.clip(cells[::3].astype(int) // 4 + 150, 0, 255).astype(np.uint8)
    sd = ref.random_state_dict_v3(2024, use_se)
    ctx.load_state_dict_v3(sd)
    out = ctx.cnn3_forward(torch.from_numpy(cells).cuda(), want_digits=True, glue=glue)
    torch.cuda.synchronize()
    logits, digits, conf = (o.cpu().numpy() for o in out)
    sel = np.arange(B) if B <= 128 else np.unique(np.concatenate([np.arange(64), np.arange(B - 64, B)]))
    lg64, _, lg32, _ = _refs(sd, cnn_oracle.glue(cells, glue)[sel])
    _check(f"u8 glue={glue} B={B} se={use_se}", logits[sel], lg64, lg32, digits[sel], conf[sel])


def _conv_of(bn_key):
    """Key of the conv weight that feeds the BatchNorm owning `bn_key`."""
    p = bn_key.rsplit(".", 1)[0]
    for bn, conv in (("stem.1", "stem.0"), ("shortcut.1", "shortcut.0"), ("bn1", "conv1"), ("bn2", "conv2")):
        if p.endswith(bn):
            return p[:-len(bn)] + conv + ".weight"
    raise KeyError(bn_key)


def _hard(name, use_se):
    sd = {k: v.clone() for k, v in ref.random_state_dict_v3(77, use_se).items()}
    if name == "var_1e-6":              # eps dominates: 1/sqrt(var + eps) = 302, not 1000.  The conv feeding such a channel is scaled with it,
        for k in list(sd):              # so that the normalised activations stay O(1)
            if k.endswith("running_var"):
                sd[k][::3] = 1e-6
                sd[_conv_of(k)][::3] *= 3e-3
    elif name == "var_1e4":
        for k in sd:
            if k.endswith("running_var"):
                sd[k][1::3] = 1e4
    elif name == "gamma_zero_negative":
        for k in sd:
            if k.endswith(".weight") and sd[k].dim() == 1:
                sd[k][::4] = 0.0
                sd[k][1::4] *= -1.0
    elif name == "se_saturated":
        for k in sd:
            if ".se.excite.2." in k:
                sd[k] *= 60.0
    elif name in ("all_1e-3", "all_1e3"):
        f = 1e-3 if name == "all_1e-3" else 1e3
        for k in sd:
            if (sd[k].dim() in (2, 4) and ".se." not in k) or k == "fc.bias":
                sd[k] *= f
    return sd


HARD = ("var_1e-6", "var_1e4", "gamma_zero_negative", "se_saturated", "all_1e-3", "all_1e3")


@pytest.mark.parametrize("name,use_se", [(n, se) for se in (True, False) for n in HARD if se or n != "se_saturated"])
def test_hard_weight_sets(ctx, name, use_se):
    sd = _hard(name, use_se)
    x = ref.inputs(9, 81)
    ctx.load_state_dict_v3(sd)
    logits, digits, conf, feats = _run(ctx, x, want_digits=True, want_features=True)
    lg64, ft64, lg32, ft32 = _refs(sd, x)
    _check(f"hard {name} se={use_se} logits", logits, lg64, lg32)
    _check(f"hard {name} se={use_se} features", feats, ft64, ft32)


def test_batch_independence_and_repeatability(ctx):
    sd, x, *_ = _pool(True)
    ctx.load_state_dict_v3(sd)
    big = _run(ctx, x[:SUB + 81])
    again = _run(ctx, x[:SUB + 81])
    assert np.array_equal(big, again)
    for i in (0, 1, 80, SUB - 1, SUB, SUB + 80):
        assert np.array_equal(_run(ctx, x[i:i + 1])[0], big[i]), i
    # a NaN cell does not disturb its neighbours
    y = x[:81].copy()
    y[40, 0, 3, 3] = np.nan
    got = _run(ctx, y)
    keep = np.arange(81) != 40
    assert np.array_equal(got[keep], big[:81][keep])


def test_temperature_in_conf(ctx):
    sd = {k: v.clone() for k, v in ref.random_state_dict_v3(2024, True).items()}
    sd["temperature"][:] = 2.5
    x = ref.inputs(5, 81)
    ctx.load_state_dict_v3(sd)
    logits, digits, conf = _run(ctx, x, want_digits=True)
    lg64, _, lg32, _ = _refs(sd, x)
    _check("temperature 2.5", logits, lg64, lg32, digits, conf, temperature=2.5)


def test_frames_to_digits_v3_is_warp_then_forward(ctx):
    import sudoku_vision_amd as sva
    from sudoku_vision_amd.synth import synth_frames
    frames, corners, _ = synth_frames(3, 270, 480, seed=4, device="cuda")
    ctx.load_state_dict_v3(ref.random_state_dict_v3(2024, True))
    minv = ctx.minv_to_device(sva.Context.corners_to_minv(corners))
    for glue in (0, 1):
        out = ctx.frames_to_digits_v3(frames, minv, keep_cells=True, glue=glue)
        cells = ctx.warp_cells(frames, minv)
        lg, dg, cf = ctx.cnn3_forward(cells.reshape(-1, 28, 28), want_digits=True, glue=glue)
        torch.cuda.synchronize()
        assert torch.equal(out["cells"].reshape(-1, 28, 28), cells.reshape(-1, 28, 28))
        assert torch.equal(out["logits"].reshape(-1, 10), lg) and torch.equal(out["digits"].reshape(-1), dg) and torch.equal(out["conf"].reshape(-1), cf)


def _dropin():
    sys.path.insert(0, os.path.join(ROOT, "sudoku-vision_amd", "ml"))
    try:
        import model_v3
    finally:
        sys.path.pop(0)
    return model_v3


@pytest.mark.parametrize("use_se", (True, False))
def test_module_dropin(ctx, use_se):
    import sudoku_vision_amd as sva
    model_v3 = _dropin()
    sd = ref.random_state_dict_v3(2024, use_se)
    m = model_v3.DigitCNNv3(use_se=use_se)
    full = {**{k: v for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")}, **sd}
    m.load_state_dict(full, strict=True)
    m = m.cuda().eval()
    x = ref.inputs(5, 33)
    xd = torch.from_numpy(x).cuda()
    lg64, ft64, lg32, ft32 = _refs(sd, x)
    pred, conf = m.get_confidence(xd)
    _check(f"module se={use_se}", m(xd).cpu().numpy(), lg64, lg32, pred.cpu().numpy(), conf.cpu().numpy())
    _check(f"module se={use_se} features", m(xd, return_features=True).cpu().numpy(), ft64, ft32)
    dctx = sva.default_context()
    key = dctx._weights_v3_key
    m(xd)
    assert dctx._weights_v3_key == key                  # nothing changed: no re-pack
    m.set_temperature(3.0)
    pred, conf = m.get_confidence(xd)
    assert dctx._weights_v3_key != key
    key = dctx._weights_v3_key
    sd3 = {k: v.cpu() for k, v in m.state_dict().items()}
    _check("module temperature 3", m(xd).cpu().numpy(), lg64, lg32, pred.cpu().numpy(), conf.cpu().numpy(), temperature=3.0)
    m.layer3.bn2.running_var.mul_(1.7)                  # a BN buffer, in place
    got = m(xd).cpu().numpy()
    assert dctx._weights_v3_key != key
    sd3 = {k: v.cpu() for k, v in m.state_dict().items()}
    lg64b, _, lg32b, _ = _refs(sd3, x)
    _check("module after BN edit", got, lg64b, lg32b)
    assert np.abs(lg64b - lg64).max() > 1e-3


def test_v1_and_v3_share_a_context(ctx):
    sd1 = cnn_oracle.random_state_dict(1234)
    sd3 = ref.random_state_dict_v3(2024, True)
    ctx.load_state_dict(sd1)
    ctx.load_state_dict_v3(sd3)
    x = torch.from_numpy(ref.inputs(5, 81)).cuda()
    a1, a3 = ctx.cnn_forward(x).clone(), ctx.cnn3_forward(x).clone()
    b1, b3 = ctx.cnn_forward(x).clone(), ctx.cnn3_forward(x).clone()
    ctx.load_state_dict_v3(ref.random_state_dict_v3(2024, False))
    c1 = ctx.cnn_forward(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(a1, b1) and torch.equal(a3, b3) and torch.equal(a1, c1)
    assert np.abs(a1.cpu().numpy() - cnn_oracle.forward(sd1, x.cpu().numpy()).numpy()).max() < 1e-4


def test_recognize_image_v3(ctx):
    import sudoku_vision_amd as sva
    from sudoku_vision_amd import pipeline
    from sudoku_vision_amd.synth import synth_frames
    import sv_oracle
    frames, _, _ = synth_frames(1, 720, 1280, seed=21, device="cpu")
    sd = ref.random_state_dict_v3(2024, True)
    image = frames[0].numpy()
    res = pipeline.recognize_image(image, model_state_dict=sd, ctx=ctx, model="v3", top_k=3)
    assert res is not None
    cells = sv_oracle.warp_cells(image, res["corners"])
    x = cnn_oracle.glue(cells, 1)
    lg64, _, lg32, _ = _refs(sd, x)
    _check("recognize_image v3", res["logits"], lg64, lg32)
    p = torch.softmax(torch.from_numpy(res["logits"]).double(), 1)          # alternatives: softmax(logits), no temperature
    top = p.topk(3, 1)
    for i in range(81):
        assert np.allclose([q for _, q in res["alternatives"][i]], top.values[i, 1:].numpy(), atol=1e-6)
    with pytest.raises(ValueError):
        pipeline.recognize_image(image, ctx=ctx, model="v2")


def test_graph_capture_after_reserve():
    import sudoku_vision_amd as sva
    c = sva.Context()
    c.load_state_dict_v3(ref.random_state_dict_v3(2024, True))
    c.reserve(SUB + 81)
    x = torch.from_numpy(ref.inputs(5, SUB + 81)).cuda()
    eager = c.cnn3_forward(x).clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c.cnn3_forward(x)                               # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = c.cnn3_forward(x)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    c.close()


def test_error_paths():
    import ctypes as C
    import sudoku_vision_amd as sva
    from sudoku_vision_amd._native import NativeError
    c = sva.Context()
    x = torch.zeros(2, 1, 28, 28, device="cuda")
    with pytest.raises(NativeError, match="SV_ERR_NO_WEIGHTS"):
        c.cnn3_forward(x)
    blob = np.zeros(700587, np.float32)
    lib = sva._native.lib()
    assert lib.sv_load_weights_v3_f32(c._h, blob.ctypes.data_as(C.c_void_p), 700587, 0) == -1       # the SE count with use_se = 0
    assert lib.sv_load_weights_v3_f32(c._h, blob.ctypes.data_as(C.c_void_p), 679595, 1) == -1
    with pytest.raises(ValueError):
        c.load_state_dict_v3(ref.random_state_dict_v3(1, True), use_se=False)
    c.load_state_dict_v3(ref.random_state_dict_v3(1, False))
    c.set_precision(c.PREC_BF16)
    with pytest.raises(NativeError, match="SV_ERR_UNSUPPORTED"):
        c.cnn3_forward(x)
    c.set_precision(c.PREC_F32)
    assert c.cnn3_forward(x).shape == (2, 10)
    c.close()
