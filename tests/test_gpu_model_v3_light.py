"""GPU (-m gpu): the DigitCNNv3Light and EmptyClassifier forwards (csrc/k12_cnn_v3_light.hip) through the C ABI via Context, against a
float64 evaluation of the unfolded models (tests/model_v3_light_ref.py).

Tolerance rule (scale-free; per batch, over the cells checked), for the logits and for Light's features:
        max|gpu - f64| <= C * max|torch_f32 - f64| + 2^-24 * max|f64|          C = C_LIGHT or C_EMPTY (model_v3_light_ref)
The noise term is the error of PyTorch-CPU's own f32 evaluation of the same unfolded model against float64.  Digits must be equal wherever
the reference's top-2 gap exceeds twice the tolerance (at most 1 % of a batch's cells may fall under that gap: asserted); conf
(softmax(logits / temperature) at the argmax) within the tolerance carried through the softmax.  is_empty must equal the reference's
decision wherever |sigmoid(logit) - threshold| exceeds the tolerance carried through the sigmoid (slope <= 1/4), same 1 % cap.
The kernels carry one cell per workgroup and have no sub-batches, so the batch sizes are 1, 2, 3, 81, one above the CU count and one above
2,000 cells, which is checked on a fixed subset: the f64 reference runs on the CPU.

C_LIGHT and C_EMPTY: about four times the largest ratio max|gpu - f64| / noise measured on an MI355X over this file, rounded up to a power
of two: C_LIGHT = 16, C_EMPTY = 8.  Measured ratios (profiles/r12_model_v3_light_accuracy.txt).  Light: 2.76 at the most (features with
every layer scaled by 1e-3), 2.61 for the logits of the one-cell batch, 2.58 in recognize_image, at most 2.4 elsewhere.  Empty: 1.51 at the
most (large negative conv biases), 1.24 for 8-bit cells through preprocess_cell, at most 1.03 elsewhere."""
import os
import sys

import numpy as np
import pytest
import torch

import cnn_oracle
import model_v3_light_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 81 * 32 + 1
SIZES = [1, 2, 3, 81, 257, BIG]
CHECKED = np.unique(np.concatenate([np.arange(258), np.arange(BIG - 64, BIG), np.arange(0, BIG, 40)]))
MAKE = {"light": ref.random_state_dict_light, "empty": ref.random_state_dict_empty}
C = {"light": "C_LIGHT", "empty": "C_EMPTY"}
_POOL = {}


def _refs(sd, x):
    lg64, ft64 = ref.forward64(sd, x, return_features=True)
    lg32, ft32 = ref.forward(sd, x, return_features=True)
    return lg64.numpy(), ft64.numpy(), lg32.numpy().astype(np.float64), ft32.numpy().astype(np.float64)


def _pool(name):
    """One pool of BIG f32 cells per model, with the f64 / f32 references of the cells in CHECKED computed once."""
    if name not in _POOL:
        sd = MAKE[name](2024)
        x = ref.inputs(5, BIG)
        _POOL[name] = (sd, x) + _refs(sd, x[CHECKED])
    return _POOL[name]


def _check(name, what, got, want, want32, digits=None, conf=None, temperature=1.0):
    noise = float(np.abs(want32 - want).max())
    tol = cnn_oracle.tolerance(want, noise, getattr(ref, C[name]))
    err = float(np.abs(got.astype(np.float64) - want).max()) if np.isfinite(got).all() else float("inf")
    print(f"ACC12 {name} {what}: err {err:.3e} noise {noise:.3e} ratio {err / max(noise, 1e-300):.3f} tol {tol:.3e}")
    assert got.shape == want.shape and err <= tol, (what, err, noise, tol)
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
    return tol


def _load(ctx, name, sd):
    (ctx.load_state_dict_v3_light if name == "light" else ctx.load_state_dict_empty)(sd)


def _np(out):
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out) if isinstance(out, tuple) else out.cpu().numpy()


def _light(ctx, x, **kw):
    return _np(ctx.cnn3_light_forward(torch.from_numpy(x).cuda(), **kw))


def _empty(ctx, x, **kw):
    return _np(ctx.empty_forward(torch.from_numpy(x).cuda(), **kw))


@pytest.mark.parametrize("B", SIZES)
def test_light_f32_over_batch_sizes(ctx, B):
    sd, x, lg64, ft64, lg32, ft32 = _pool("light")
    _load(ctx, "light", sd)
    logits, digits, conf, feats = _light(ctx, x[:B], want_digits=True, want_features=True)
    sel = CHECKED[CHECKED < B]
    k = np.searchsorted(CHECKED, sel)
    _check("light", f"f32 B={B} logits", logits[sel], lg64[k], lg32[k], digits[sel], conf[sel])
    _check("light", f"f32 B={B} features", feats[sel], ft64[k], ft32[k])


def _check_is_empty(what, logit, want, tol):
    p_want = 1.0 / (1.0 + np.exp(-want))
    for thr in (0.5, 0.9):
        clear = np.abs(p_want - thr) > 0.25 * tol + 1e-7                 # sigmoid's slope is at most 1/4; 1e-7: torch.sigmoid's own f32 rounding
        assert (~clear).sum() <= 0.01 * len(want), (what, thr, int((~clear).sum()))
        got = (torch.sigmoid(torch.from_numpy(logit)) < thr).numpy()     # is_empty, as the reference writes it
        assert (got[clear] == (p_want < thr)[clear]).all(), (what, thr)
        assert 0 < got.sum() < got.size or len(want) < 20


@pytest.mark.parametrize("B", SIZES)
def test_empty_f32_over_batch_sizes(ctx, B):
    sd, x, lg64, _, lg32, _ = _pool("empty")
    _load(ctx, "empty", sd)
    logit = _empty(ctx, x[:B])
    assert logit.shape == (B, 1)
    sel = CHECKED[CHECKED < B]
    k = np.searchsorted(CHECKED, sel)
    tol = _check("empty", f"f32 B={B} logit", logit[sel], lg64[k], lg32[k])
    if B >= 81:
        _check_is_empty(f"B={B}", logit[sel], lg64[k], tol)


@pytest.mark.parametrize("glue", (0, 1))
@pytest.mark.parametrize("B", (81, 259))
def test_u8_cells(ctx, B, glue):
    rs = np.random.RandomState(B + glue)
    cells = rs.randint(0, 256, (B, 28, 28)).astype(np.uint8)
    cells[::3] = np.clip(cells[::3].astype(int) // 4 + 150, 0, 255).astype(np.uint8)
    xd = torch.from_numpy(cells).cuda()
    x = cnn_oracle.glue(cells, glue)
    sd = MAKE["light"](2024)
    _load(ctx, "light", sd)
    logits, digits, conf = _np(ctx.cnn3_light_forward(xd, want_digits=True, glue=glue))
    lg64, _, lg32, _ = _refs(sd, x)
    _check("light", f"u8 glue={glue} B={B}", logits, lg64, lg32, digits, conf)
    with pytest.raises(ValueError):
        ctx.cnn3_light_forward(xd, want_features=True)
    sd = MAKE["empty"](2024)
    _load(ctx, "empty", sd)
    lg64, _, lg32, _ = _refs(sd, x)
    _check("empty", f"u8 glue={glue} B={B}", _np(ctx.empty_forward(xd, glue=glue)), lg64, lg32)


def _hard(model, name):
    sd = {k: v.clone() for k, v in MAKE[model](77).items()}
    conv_of = {"features.1": "features.0.weight", "features.5": "features.4.weight", "features.9": "features.8.weight"}
    if name == "var_1e-6":              # eps dominates: 1/sqrt(var + eps) = 302, not 1000.  The conv feeding such a channel is scaled with it
        for k in list(sd):
            if k.endswith("running_var"):
                sd[k][::3] = 1e-6
                sd[conv_of[k.rsplit(".", 1)[0]]][::3] *= 3e-3
    elif name == "var_1e4":
        for k in sd:
            if k.endswith("running_var"):
                sd[k][1::3] = 1e4
    elif name == "gamma_zero_negative":
        for k in ("features.1.weight", "features.5.weight", "features.9.weight"):
            sd[k][::4] = 0.0
            sd[k][1::4] *= -1.0
    elif name == "negative_conv_bias":  # whole pooled planes are zero: ReLU clips every pixel of these channels
        sd["features.0.bias"][::2] = -50.0
        sd["features.3.bias"][1::3] = -500.0
    elif name in ("all_1e-3", "all_1e3"):
        f = 1e-3 if name == "all_1e-3" else 1e3
        for k in sd:
            if sd[k].dim() in (2, 4) or k in ("fc.bias", "classifier.4.bias"):
                sd[k] *= f
    return sd


HARD = [("light", n) for n in ("var_1e-6", "var_1e4", "gamma_zero_negative", "all_1e-3", "all_1e3")] + \
       [("empty", n) for n in ("negative_conv_bias", "all_1e-3", "all_1e3")]


@pytest.mark.parametrize("model,name", HARD)
def test_hard_weight_sets(ctx, model, name):
    sd = _hard(model, name)
    x = ref.inputs(9, 81)
    _load(ctx, model, sd)
    lg64, ft64, lg32, ft32 = _refs(sd, x)
    if model == "light":
        logits, feats = _light(ctx, x, want_features=True)
        _check(model, f"hard {name} logits", logits, lg64, lg32)
        _check(model, f"hard {name} features", feats, ft64, ft32)
    else:
        if name == "negative_conv_bias":
            assert (ft64.reshape(81, 32, 49)[:, 1::3] == 0).all()
        _check(model, f"hard {name} logit", _empty(ctx, x), lg64, lg32)


def test_batch_independence_and_repeatability(ctx):
    for name, run in (("light", _light), ("empty", _empty)):
        sd, x, *_ = _pool(name)
        _load(ctx, name, sd)
        big = run(ctx, x)
        again = run(ctx, x)
        assert np.array_equal(big, again)
        for i in (0, 1, 80, 256, 257, BIG - 1):
            assert np.array_equal(run(ctx, x[i:i + 1])[0], big[i]), (name, i)
        assert np.array_equal(run(ctx, x[100:300]), big[100:300])
        # a NaN cell does not disturb its neighbours
        y = x[:81].copy()
        y[40, 0, 3, 3] = np.nan
        got = run(ctx, y)
        keep = np.arange(81) != 40
        assert np.array_equal(got[keep], big[:81][keep])


def test_temperature_in_conf(ctx):
    sd = {k: v.clone() for k, v in MAKE["light"](2024).items()}
    sd["temperature"][:] = 2.5
    x = ref.inputs(5, 81)
    _load(ctx, "light", sd)
    logits, digits, conf = _light(ctx, x, want_digits=True)
    lg64, _, lg32, _ = _refs(sd, x)
    _check("light", "temperature 2.5", logits, lg64, lg32, digits, conf, temperature=2.5)


def test_four_models_share_a_context():
    import model_v3_ref
    import sudoku_vision_amd as sva
    sds = {"v1": cnn_oracle.random_state_dict(1234), "v3": model_v3_ref.random_state_dict_v3(2024, True),
           "light": MAKE["light"](2024), "empty": MAKE["empty"](2024)}
    load = {"v1": "load_state_dict", "v3": "load_state_dict_v3", "light": "load_state_dict_v3_light", "empty": "load_state_dict_empty"}
    fwd = {"v1": "cnn_forward", "v3": "cnn3_forward", "light": "cnn3_light_forward", "empty": "empty_forward"}
    x = torch.from_numpy(ref.inputs(5, 81)).cuda()
    alone = {}
    for m in sds:
        c = sva.Context()
        getattr(c, load[m])(sds[m])
        alone[m] = getattr(c, fwd[m])(x).clone()
        torch.cuda.synchronize()
        c.close()
    c = sva.Context()
    for m in sds:
        getattr(c, load[m])(sds[m])
    for m in sds:
        assert torch.equal(getattr(c, fwd[m])(x), alone[m]), m
    c.load_state_dict_v3_light(MAKE["light"](77))
    assert not torch.equal(c.cnn3_light_forward(x), alone["light"])
    for m in ("v1", "v3", "empty"):
        assert torch.equal(getattr(c, fwd[m])(x), alone[m]), m
    c.load_state_dict_empty(MAKE["empty"](77))
    c.load_state_dict_v3_light(sds["light"])
    for m in ("v1", "v3", "light"):
        assert torch.equal(getattr(c, fwd[m])(x), alone[m]), m
    torch.cuda.synchronize()
    c.close()


def test_frames_to_digits_v3_light_is_warp_then_forward(ctx):
    import sudoku_vision_amd as sva
    from sudoku_vision_amd.synth import synth_frames
    frames, corners, _ = synth_frames(3, 270, 480, seed=4, device="cuda")
    _load(ctx, "light", MAKE["light"](2024))
    minv = ctx.minv_to_device(sva.Context.corners_to_minv(corners))
    for glue in (0, 1):
        out = ctx.frames_to_digits_v3_light(frames, minv, keep_cells=True, glue=glue)
        cells = ctx.warp_cells(frames, minv)
        lg, dg, cf = ctx.cnn3_light_forward(cells.reshape(-1, 28, 28), want_digits=True, glue=glue)
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


def test_module_dropin_light(ctx):
    import sudoku_vision_amd as sva
    model_v3 = _dropin()
    sd = MAKE["light"](2024)
    m = model_v3.DigitCNNv3Light()
    m.load_state_dict({**{k: v for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")}, **sd}, strict=True)
    m = m.cuda().eval()
    x = ref.inputs(5, 33)
    xd = torch.from_numpy(x).cuda()
    lg64, _, lg32, _ = _refs(sd, x)
    pred, conf = m.get_confidence(xd)
    assert pred.dtype == torch.int64
    _check("light", "module", m(xd).cpu().numpy(), lg64, lg32, pred.cpu().numpy(), conf.cpu().numpy())
    dctx = sva.default_context()
    dctx.load_state_dict_v3_light(sd, key=dctx._weights_light_key)
    assert torch.equal(m(xd), dctx.cnn3_light_forward(xd))
    key = dctx._weights_light_key
    m(xd)
    assert dctx._weights_light_key == key                 # nothing changed: no re-pack
    m.set_temperature(3.0)
    pred, conf = m.get_confidence(xd)
    assert dctx._weights_light_key != key
    key = dctx._weights_light_key
    _check("light", "module temperature 3", m(xd).cpu().numpy(), lg64, lg32, pred.cpu().numpy(), conf.cpu().numpy(), temperature=3.0)
    m.features[5].running_var.mul_(1.7)                   # a BN buffer, in place
    got = m(xd).cpu().numpy()
    assert dctx._weights_light_key != key
    sd3 = {k: v.cpu() for k, v in m.state_dict().items()}
    lg64b, _, lg32b, _ = _refs(sd3, x)
    _check("light", "module after BN edit", got, lg64b, lg32b)
    assert np.abs(lg64b - lg64).max() > 1e-3
    with pytest.raises(NotImplementedError):
        m.train()(xd)


def test_module_dropin_empty(ctx):
    import sudoku_vision_amd as sva
    model_v3 = _dropin()
    sd = MAKE["empty"](2024)
    m = model_v3.EmptyClassifier()
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    x = ref.inputs(5, 200)
    xd = torch.from_numpy(x).cuda()
    lg64, _, lg32, _ = _refs(sd, x)
    got = m(xd)
    tol = _check("empty", "module", got.cpu().numpy(), lg64, lg32)
    _check_is_empty("module", got.cpu().numpy(), lg64, tol)
    for thr in (0.5, 0.9):
        e = m.is_empty(xd, thr)
        assert e.is_cuda and e.dtype == torch.bool and e.shape == (200, 1)
        assert torch.equal(e, torch.sigmoid(got) < thr)
    assert torch.equal(m.is_empty(xd), m.is_empty(xd, 0.5))
    dctx = sva.default_context()
    key = dctx._weights_empty_key
    m(xd)
    assert dctx._weights_empty_key == key
    with torch.no_grad():
        m.classifier[4].bias.add_(1.0)
    assert np.allclose((m(xd) - got).cpu().numpy(), 1.0, atol=1e-5) and dctx._weights_empty_key != key


def test_recognize_image_v3_light(ctx):
    from sudoku_vision_amd import pipeline
    from sudoku_vision_amd.synth import synth_frames
    import sv_oracle
    frames, _, _ = synth_frames(1, 720, 1280, seed=21, device="cpu")
    sd = MAKE["light"](2024)
    image = frames[0].numpy()
    res = pipeline.recognize_image(image, model_state_dict=sd, ctx=ctx, model="v3_light", top_k=3, resolve=True, propagate=True)
    assert res is not None
    cells = sv_oracle.warp_cells(image, res["corners"])
    lg64, _, lg32, _ = _refs(sd, cnn_oracle.glue(cells, 1))
    _check("light", "recognize_image v3_light", res["logits"], lg64, lg32)
    # the same call, assembled from the forward on the kept cells
    lg, dg, cf = ctx.cnn3_light_forward(torch.from_numpy(cells.reshape(81, 28, 28)).cuda(), want_digits=True, glue=1)
    assert np.array_equal(res["logits"], lg.cpu().numpy()) and np.array_equal(res["digits"], dg.cpu().numpy())
    assert np.array_equal(res["confidence"], cf.cpu().numpy())
    idx, prob = ctx.softmax_topk(lg, 3)
    want = pipeline._validate_and_resolve(ctx, idx[None], prob[None])
    resolved = want.pop("_cells")
    for k in want:
        assert res[k] == want[k], k
    state = {k: v[0].cpu().numpy() for k, v in ctx.propagate_constraints(*resolved).items()}
    assert res["propagated_grid"] == [[int(state["grid"][r * 9 + c]) for c in range(9)] for r in range(9)]
    assert res["propagation"]["is_valid"] == bool(state["is_valid"]) and res["propagation"]["iterations"] == int(state["iterations"])
    p = torch.softmax(torch.from_numpy(res["logits"]).double(), 1).topk(3, 1)
    for i in range(81):
        assert np.allclose([q for _, q in res["alternatives"][i]], p.values[i, 1:].numpy(), atol=1e-6)
    with pytest.raises(ValueError):
        pipeline.recognize_image(image, ctx=ctx, model="v3_lite")


def test_graph_capture_after_reserve():
    import sudoku_vision_amd as sva
    c = sva.Context()
    c.load_state_dict_v3_light(MAKE["light"](2024))
    c.reserve(81)
    c.load_state_dict_empty(MAKE["empty"](2024))          # a load after the reserve
    x = torch.from_numpy(ref.inputs(5, 81)).cuda()
    u8 = torch.randint(0, 256, (81, 28, 28), dtype=torch.uint8, device="cuda")
    eager = [c.cnn3_light_forward(x).clone(), c.empty_forward(x).clone(), c.cnn3_light_forward(u8, glue=1).clone()]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c.cnn3_light_forward(x)                           # warm-up on the side stream
        c.empty_forward(x)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = [c.cnn3_light_forward(x), c.empty_forward(x), c.cnn3_light_forward(u8, glue=1)]
    for _ in range(2):
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        for o, e in zip(outs, eager):
            assert torch.equal(o, e)
    c.close()


def test_error_paths():
    import ctypes as C
    import sudoku_vision_amd as sva
    from sudoku_vision_amd._native import NativeError
    c = sva.Context()
    x = torch.zeros(2, 1, 28, 28, device="cuda")
    with pytest.raises(NativeError, match="SV_ERR_NO_WEIGHTS"):
        c.cnn3_light_forward(x)
    with pytest.raises(NativeError, match="SV_ERR_NO_WEIGHTS"):
        c.empty_forward(x)
    with pytest.raises(NativeError, match="SV_ERR_NO_WEIGHTS"):
        c.frames_to_digits_v3_light(torch.zeros(1, 270, 480, 3, dtype=torch.uint8, device="cuda"), torch.eye(3, dtype=torch.float64, device="cuda")[None])
    blob = np.zeros(60000, np.float32)
    lib = sva._native.lib()
    for n in (53698, 53700, 55041):
        assert lib.sv_load_weights_v3_light_f32(c._h, blob.ctypes.data_as(C.c_void_p), n) == -1
    for n in (55040, 55042, 53699):
        assert lib.sv_load_weights_empty_f32(c._h, blob.ctypes.data_as(C.c_void_p), n) == -1
    with pytest.raises(NativeError, match="SV_ERR_BAD_ARG"):
        c._check(lib.sv_load_weights_empty_f32(c._h, blob.ctypes.data_as(C.c_void_p), 7), "sv_load_weights_empty_f32")
    with pytest.raises(ValueError, match="not DigitCNNv3Light keys"):
        c.load_state_dict_v3_light({**MAKE["light"](1), "layer1.conv1.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match="not EmptyClassifier keys"):
        c.load_state_dict_empty({**MAKE["empty"](1), "fc.weight": torch.zeros(1)})
    with pytest.raises(KeyError):
        c.load_state_dict_empty({})
    c.load_state_dict_v3_light({**MAKE["light"](1), "features.1.num_batches_tracked": torch.zeros((), dtype=torch.int64)})
    c.load_state_dict_empty(MAKE["empty"](1))
    c.set_precision(c.PREC_BF16)
    with pytest.raises(NativeError, match="SV_ERR_UNSUPPORTED"):
        c.cnn3_light_forward(x)
    with pytest.raises(NativeError, match="SV_ERR_UNSUPPORTED"):
        c.empty_forward(x)
    c.set_precision(c.PREC_F32)
    assert c.cnn3_light_forward(x).shape == (2, 10) and c.empty_forward(x).shape == (2, 1)
    lg, dg, cf = c.cnn3_light_forward(x[:0], want_digits=True)          # B = 0 is accepted
    assert lg.shape == (0, 10) and dg.shape == (0,) and c.empty_forward(x[:0]).shape == (0, 1)
    torch.cuda.synchronize()
    c.close()
