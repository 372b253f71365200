"""GPU (-m gpu): every CNN kernel family against a float64 evaluation of the model (oracle/cnn_oracle.py), at the batch sizes where the
launch code changes shape, over weight scales from 1e-6 to 1e11 and at the f32-input range switch points.

Tolerance rule (scale-free; per batch, over the cells checked):
  f32 families -- SV_CNN_AUTO, SV_CNN_F16PAIR, SV_CNN_F32MFMA and the test-only library's Winograd (f32 MFMA), split-bf16 Winograd and
  frame-per-workgroup fc kernels:
        max|gpu - f64| <= C_F32 * max|torch_f32 - f64| + 2^-24 * max|f64|
  bf16 configuration (its own operands are bf16, so the reference is the emulation of its rounding points, forward_bf16_emulated):
        max|gpu - emu64| <= C_BF16 * max|emu_f32acc - emu64| + 2^-24 * max|emu64|
  The first term is what another f32-summing evaluation of the same operands gets wrong; both terms scale with the weights and the
  inputs, so the rule is as tight at 1e-6 as at 1e6.  C_F32 = 56, C_BF16 = 52 (cnn_oracle): about four times the largest ratio
  max|gpu - ref| / noise measured on an MI355X over this file.  f32 families: at most 3.1 with the trained and random weights, 2.6 with
  the run.py glue, 3.9 at the input switch points, and 9.7 with every layer scaled by 1e-3 (8.1 with conv1 by 1e-6): there the logits or
  the features are almost all bias, and the kernels, which start every fc2 sum from the bias, round after each of 128 tiny terms where
  PyTorch adds the bias once at the end -- the same ratio for every family, since they share that epilogue (13.1 with fc1 by 1e-6, and
  with the mix (1e-3, 1e3, 1e-6, 1e6), after the activation scaling went in).  bf16 (8-bit glue): at most 7 with the trained and random
  weights, 12.6 over the weight scales (the same bias-dominated cases); the run.py glue: see test_bf16_over_batch_sizes.
  Digits must be equal wherever the reference's top-2 gap exceeds twice the tolerance; conf (softmax at the argmax) within the tolerance
  carried through the softmax: a shift of every logit by at most tol moves it by at most a factor exp(+-2 tol), plus f32 rounding.
Large batches are checked on a fixed subset (first and last 128 cells and every k-th): the f64 reference runs on the CPU."""
import os

import numpy as np
import pytest
import torch

import cnn_oracle

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 15, 16, 17, 63, 64, 65, 81 * 64 - 1, 81 * 64 + 1, 96 * 256, 96 * 256 + 1]
SCALES = {                          # per-layer (conv1, conv2, fc1, fc2) factors on weight and bias
    "1": (1, 1, 1, 1), "all_1e-6": (1e-6,) * 4, "all_1e-3": (1e-3,) * 4, "all_1e3": (1e3,) * 4, "all_1e6": (1e6,) * 4,
    "c1_1e-6": (1e-6, 1, 1, 1), "c1_1e6": (1e6, 1, 1, 1), "c2_1e-6": (1, 1e-6, 1, 1), "c2_1e6": (1, 1e6, 1, 1),
    "f1_1e-6": (1, 1, 1e-6, 1), "f1_1e6": (1, 1, 1e6, 1), "f2_1e-6": (1, 1, 1, 1e-6), "f2_1e6": (1, 1, 1, 1e6),
    "mix_a": (1e6, 1e-6, 1, 1), "mix_b": (1e-6, 1e6, 1e-3, 1e3), "mix_c": (1e-3, 1e3, 1e-6, 1e6), "mix_d": (1e3, 1e-3, 1e6, 1e-6),
}
_REPORT = []


def _sd(name, golden_dir):
    if name == "trained":
        g = np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz"))
        return {k: torch.from_numpy(g[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS}
    return {k: v.clone() for k, v in cnn_oracle.random_state_dict(1234).items()}


def _cells(n, seed):
    rs = np.random.RandomState(seed)
    cells = rs.randint(0, 256, (n, 28, 28)).astype(np.uint8)
    cells[::3] = np.clip(cells[::3].astype(int) // 4 + 150, 0, 255).astype(np.uint8)
    return cells


def _subset(B):
    k = max(1, B // 128)
    return np.unique(np.concatenate([np.arange(min(128, B)), np.arange(max(0, B - 128), B), np.arange(0, B, k)]))


def _check(what, out, want, noise, c, slack=0.0):
    """out = (logits, digits, conf) of the checked cells (numpy); want = float64 reference logits of the same cells; slack: an extra
    allowance, times max|want| (cnn_oracle.BF16_RUNPY_SLACK)."""
    logits, digits, conf = out
    tol = cnn_oracle.tolerance(want, noise, c) + slack * float(np.abs(want).max())
    err = float(np.abs(logits.astype(np.float64) - want).max()) if np.isfinite(logits).all() else float("inf")
    _REPORT.append((what, err, float(noise), tol))
    print(f"ACC {what}: err {err:.3e} noise {noise:.3e} ratio {err / max(noise, 1e-300):.3f} tol {tol:.3e}")
    assert err <= tol, (what, err, noise, tol)
    top2 = np.sort(want, 1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 2 * tol
    assert (digits[clear] == want.argmax(1)[clear]).all(), what
    e = np.exp(want - want.max(1, keepdims=True))
    conf_want = 1.0 / e.sum(1)
    assert (np.abs(conf - conf_want) <= conf_want * np.expm1(min(2 * tol, 50.0)) + 2e-6).all(), what


class _F32Ref:
    """float64 and PyTorch-f32 logits of the cells `idx` of one f32 input array, computed once per cell."""

    def __init__(self, sd, x):
        self.sd, self.x, self.f64, self.t32 = sd, x, {}, {}

    def get(self, idx):
        todo = np.array([i for i in idx if i not in self.f64], dtype=np.int64)
        if todo.size:
            f, t = cnn_oracle.forward64(self.sd, self.x[todo]).numpy(), cnn_oracle.forward(self.sd, self.x[todo]).numpy()
            for j, i in enumerate(todo):
                self.f64[i], self.t32[i] = f[j], t[j]
        want = np.stack([self.f64[i] for i in idx])
        return want, float(np.abs(np.stack([self.t32[i] for i in idx]) - want).max())


def _contexts():
    """(name, context, selection, frame fc) of every f32 family; the last three are the test-only library's."""
    import sudoku_vision_amd as sva
    prod, xc = sva.Context(), sva.Context(library=sva._native.lib_xcheck())
    fams = [("auto", prod, prod.CNN_AUTO, 0), ("f16pair", prod, prod.CNN_F16PAIR, 0), ("f32mfma", prod, prod.CNN_F32MFMA, 0),
            ("winograd", xc, xc.CNN_X_WINOGRAD, 0), ("wsplit", xc, xc.CNN_X_WSPLIT, 0), ("frame_fc", xc, xc.CNN_F32MFMA, 1),
            ("auto_frame_fc", xc, xc.CNN_AUTO, 1)]
    return prod, xc, fams


def _run(c, which, frame, x, glue=0):
    c.set_cnn_kernels(which)
    if frame is not None and hasattr(c._lib, "svx_ctx_set_fc_frame_kernel"):
        c._check(c._lib.svx_ctx_set_fc_frame_kernel(c._h, frame), "svx_ctx_set_fc_frame_kernel")
    return c.cnn_forward(x, want_digits=True, glue=glue)


def _host(out, idx):
    return tuple(t.cpu().numpy()[idx] for t in out)


@pytest.mark.parametrize("weights", ["trained", "random"])
def test_f32_families_over_batch_sizes(golden_dir, weights):
    """Every f32 family, 8-bit cells (the glue fused in) and the same cells as f32 input, at each tail and dispatch boundary of the launch
    code: 1-3 cells, the 16-cell M tiles and 64-cell fc workgroups (15-17, 63-65), the frame fc kernel's 81*64 threshold, and the last
    one-pass batch of the per-CU fc kernel (96 cells per CU) and the first past it.  auto_frame_fc is SV_CNN_AUTO with the frame fc kernel
    switched on, whose f32-input batches used to be overwritten by that kernel after the f16-pair kernels had written them."""
    sd = _sd(weights, golden_dir)
    cells = _cells(SIZES[-1], 11)
    x = cnn_oracle.glue(cells)
    ref = _F32Ref(sd, x)
    prod, xc, fams = _contexts()
    prod.load_state_dict(sd)
    xc.load_state_dict(sd)
    d8, d32 = torch.from_numpy(cells).cuda(), torch.from_numpy(x).cuda()
    for B in SIZES:
        idx = _subset(B)
        want, noise = ref.get(idx)
        for name, c, which, frame in fams:
            for form, data in (("u8", d8), ("f32", d32)):
                _check(f"{weights} {name} {form} B={B}", _host(_run(c, which, frame, data[:B]), idx), want, noise, cnn_oracle.C_F32)
    prod.close()
    xc.close()


def test_f32_families_runpy_glue(golden_dir):
    """The run.py glue (preprocess_cell first) on every f32 family."""
    sd = _sd("trained", golden_dir)
    cells = _cells(81 * 64 + 1, 12)
    prod, xc, fams = _contexts()
    prod.load_state_dict(sd)
    xc.load_state_dict(sd)
    d8 = torch.from_numpy(cells).cuda()
    for B in (1, 17, 65, 81 * 64 + 1):
        idx = _subset(B)
        x = cnn_oracle.glue(cells[idx], 1)
        want = cnn_oracle.forward64(sd, x).numpy()
        noise = np.abs(cnn_oracle.forward(sd, x).numpy() - want).max()
        for name, c, which, frame in fams:
            _check(f"runpy {name} B={B}", _host(_run(c, which, frame, d8[:B], glue=1), idx), want, noise, cnn_oracle.C_F32)
    prod.close()
    xc.close()


@pytest.mark.parametrize("weights", ["trained", "random"])
def test_bf16_over_batch_sizes(golden_dir, weights):
    """The bf16 configuration at the same sizes (the conv kernel takes two cells per workgroup: the odd sizes leave one alone; 96*256 is also
    its k_fc_head_bf16p / k_fc_head_bf16 boundary), both glues, against the emulation of its rounding points.  The noise term is taken over
    all cells this test checks (a bf16 rounding that an f32 sum tips the other way moves a logit by far more than f32 noise, and such
    events are rare: the larger the sample, the truer the estimate).  With the run.py glue the bound carries cnn_oracle.BF16_RUNPY_SLACK:
    measured there, 8e-4 against a noise term of 4e-6 (trained weights; binary inputs make the f32 sums nearly exact, so the noise term
    is tiny, while a bf16 rounding tie decided the other way is not; see cnn_oracle)."""
    import sudoku_vision_amd as sva
    sd = _sd(weights, golden_dir)
    cells = _cells(SIZES[-1], 13)
    c = sva.Context()
    c.load_state_dict(sd)
    c.set_precision(c.PREC_BF16)
    d8 = torch.from_numpy(cells).cuda()
    idx_all = np.unique(np.concatenate([_subset(B) for B in SIZES]))
    pos = {i: j for j, i in enumerate(idx_all)}
    for glue in (0, 1):
        emu = cnn_oracle.forward_bf16_emulated(sd, cells[idx_all], glue).numpy()
        noise = np.abs(cnn_oracle.forward_bf16_emulated(sd, cells[idx_all], glue, acc=torch.float32).numpy() - emu).max()
        for B in (SIZES if glue == 0 else (1, 2, 17, 65, 96 * 256 + 1)):
            idx = _subset(B)
            sel = np.array([pos[i] for i in idx])
            _check(f"{weights} bf16 glue{glue} B={B}", _host(c.cnn_forward(d8[:B], want_digits=True, glue=glue), idx), emu[sel], noise,
                   cnn_oracle.C_BF16, cnn_oracle.BF16_RUNPY_SLACK if glue == 1 else 0.0)
    c.close()


def _scaled(kind, golden_dir):
    sd = _sd("random", golden_dir)
    if kind == "fc1w_1e11":                     # the weight-range case: fc1's weights alone
        sd["fc1.weight"] *= 1e11
    elif kind == "c1_tiny_c2_huge":             # conv1's activations ~1e-11, conv2's weights up to 2e9
        sd["conv1.weight"] *= 1e-11
        sd["conv1.bias"] *= 1e-11
        sd["conv2.weight"] *= 2e9 / float(sd["conv2.weight"].abs().max())
    else:
        for layer, f in zip(("conv1", "conv2", "fc1", "fc2"), SCALES[kind]):
            sd[layer + ".weight"] *= f
            sd[layer + ".bias"] *= f
    return sd


@pytest.mark.parametrize("kind", list(SCALES) + ["fc1w_1e11", "c1_tiny_c2_huge"])
def test_weight_scales(golden_dir, kind):
    """Random weights with independent per-layer scales (weights and biases together) from 1e-6 to 1e6, fc1's weights x 1e11 and the
    conv1-tiny / conv2-huge set: every f32 family (the f16-pair kernels forced only where the loader finds them in range -- asserted to be
    where sv_load_weights_f32 puts SV_CNN_AUTO) on 8-bit cells and f32 input, and the bf16 configuration."""
    import sudoku_vision_amd as sva
    sd = _scaled(kind, golden_dir)
    rng = cnn_oracle.pair_range(sd)
    cells = _cells(65, 14)
    xs = {"u8": cnn_oracle.glue(cells), "f32": np.random.RandomState(15).uniform(-1, 1, (65, 1, 28, 28)).astype(np.float32)}
    refs = {}
    for form, x in xs.items():
        want = cnn_oracle.forward64(sd, x).numpy()
        assert np.isfinite(want).all()
        refs[form] = (want, np.abs(cnn_oracle.forward(sd, x).numpy() - want).max())
    prod, xc, fams = _contexts()
    prod.load_state_dict(sd)
    xc.load_state_dict(sd)
    assert prod.conv_kernel_info()["algo"] == (4 if rng["in_range"] else 0), rng
    if kind in ("fc1w_1e11", "c1_tiny_c2_huge", "1"):
        assert rng["in_range"]                  # the default kernels serve these
    idx = np.arange(65)
    data = {"u8": torch.from_numpy(cells).cuda(), "f32": torch.from_numpy(xs["f32"]).cuda()}
    for name, c, which, frame in fams:
        if name == "f16pair" and not rng["in_range"]:
            continue
        for form in ("u8", "f32"):
            _check(f"scale {kind} {name} {form}", _host(_run(c, which, frame, data[form]), idx), *refs[form], cnn_oracle.C_F32)
    prod.close()
    xc.close()
    b = sva.Context()
    b.load_state_dict(sd)
    b.set_precision(b.PREC_BF16)
    more = _cells(4 * 65, 14)                  # (its first 65 are `cells`): the noise term over four times the cells checked
    assert np.array_equal(more[:65], cells)
    emu = cnn_oracle.forward_bf16_emulated(sd, more).numpy()
    noise = np.abs(cnn_oracle.forward_bf16_emulated(sd, more, acc=torch.float32).numpy() - emu).max()
    _check(f"scale {kind} bf16", _host(b.cnn_forward(data["u8"], want_digits=True), idx), emu[:65], noise, cnn_oracle.C_BF16)
    b.close()


def test_f32_input_switch_points(golden_dir):
    """f32 batches whose max|x| sits at the edges of the f16-pair kernels' input range (h2_x_lo = 2^-3, h2_x_hi restated from
    sv_load_weights_f32 by cnn_oracle.pair_range), an all-zero batch and a batch with one non-zero element.  SV_CNN_AUTO must meet the
    tolerance everywhere and must have taken the kernels the range names: its logits equal, bit for bit, those of the f16-pair kernels
    forced (inside) or of the f32-MFMA kernels forced (outside).  What the forced f16-pair kernels give below 2^-3 is reported, not
    asserted: there an unscaled input's low halves are f16-subnormal."""
    import sudoku_vision_amd as sva
    sd = _sd("random", golden_dir)
    rng = cnn_oracle.pair_range(sd)
    lo, hi = rng["x_lo"], rng["x_hi"]
    base = np.random.RandomState(16).uniform(-1, 1, (65, 1, 28, 28)).astype(np.float32)
    peak = int(np.abs(base).argmax())
    points = {"2^-10(1-2^-10)": 2.0 ** -10 * (1 - 2.0 ** -10), "2^-10(1+2^-10)": 2.0 ** -10 * (1 + 2.0 ** -10), "lo(1-2^-10)": lo * (1 - 2.0 ** -10),
              "lo": lo, "1": 1.0, "hi(1-1e-3)": hi * (1 - 1e-3), "hi(1+1e-3)": hi * (1 + 1e-3)}
    cases = {}
    for name, m in points.items():
        x = (base * np.float32(m / np.abs(base).max())).astype(np.float32)
        x.flat[peak] = np.float32(m) * np.sign(x.flat[peak])
        cases[name] = x
    cases["zeros"] = np.zeros_like(base)
    one = np.zeros_like(base)
    one[7, 0, 13, 14] = 0.75
    cases["single"] = one
    c = sva.Context()
    c.load_state_dict(sd)
    for name, x in cases.items():
        m = float(np.abs(x).max())
        inside = lo <= m <= hi
        want = cnn_oracle.forward64(sd, x).numpy()
        noise = np.abs(cnn_oracle.forward(sd, x).numpy() - want).max()
        d, every = torch.from_numpy(x).cuda(), np.arange(65)
        auto, pair, f32 = (_run(c, which, None, d) for which in (c.CNN_AUTO, c.CNN_F16PAIR, c.CNN_F32MFMA))
        assert torch.equal(auto[0], (pair if inside else f32)[0]), (name, m, inside)
        _check(f"switch {name} auto", _host(auto, every), want, noise, cnn_oracle.C_F32)
        _check(f"switch {name} f32mfma", _host(f32, every), want, noise, cnn_oracle.C_F32)
        if inside:
            _check(f"switch {name} f16pair", _host(pair, every), want, noise, cnn_oracle.C_F32)
        elif m <= hi:
            err = float(np.abs(pair[0].cpu().numpy() - want).max())
            print(f"ACC-INFO switch {name} f16pair forced below its range: err {err:.3e} noise {noise:.3e} ratio {err / max(noise, 1e-300):.3f}")
    c.close()


@pytest.fixture(scope="module", autouse=True)
def _largest_ratios(ctx):                   # (ctx: skips the module without a GPU)
    """Prints the largest measured ratio max|gpu - ref| / noise per family when the module is done (visible with -s): the calibration of
    C_F32 / C_BF16."""
    yield
    worst = {}
    for what, err, noise, tol in _REPORT:
        fam = "bf16" if "bf16" in what else what.split()[2] if what.startswith(("scale", "switch")) else what.split()[1]
        worst[fam] = max(worst.get(fam, 0.0), err / max(noise, 1e-300))
    for fam, r in sorted(worst.items()):
        print(f"ACC-MAX {fam}: ratio {r:.3f}")
