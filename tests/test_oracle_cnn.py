"""CPU: the torch restatement of DigitCNN (oracle/cnn_oracle.py) against goldens captured from the
reference's own ml/model.py (tests/golden/make_goldens.py); the float64 reference, the emulations of the reduced-operand
kernels and the tolerance rule the GPU accuracy tests use."""
import os

import numpy as np
import pytest
import torch

import cnn_oracle


def _coreml_sd(g):
    return {k: torch.from_numpy(g[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS}


def test_random_weights_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "cnn_random_seed1234.npz"))
    sd = cnn_oracle.random_state_dict(int(g["seed"]))
    x = cnn_oracle.golden_inputs(int(g["x_seed"]), 81)
    logits = cnn_oracle.forward(sd, x).numpy()
    assert np.abs(logits - g["logits"]).max() <= 1e-5
    assert (logits.argmax(1) == g["digits"]).all()


def test_trained_weights_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz"))
    sd = _coreml_sd(g)
    assert sum(v.numel() for v in sd.values()) == 421642
    x = cnn_oracle.golden_inputs(int(g["x_seed"]), 162)
    logits, digits, conf = cnn_oracle.predict(sd, x)
    assert np.abs(logits.numpy() - g["logits"]).max() <= 1e-4
    assert (digits.numpy() == g["digits"]).all()
    assert ((conf > 0) & (conf <= 1)).all()


def test_batch_independence():
    sd = cnn_oracle.random_state_dict(1)
    x = cnn_oracle.golden_inputs(2, 16)
    a = cnn_oracle.forward(sd, x).numpy()
    b = np.concatenate([cnn_oracle.forward(sd, x[i:i + 1]).numpy() for i in range(16)])
    assert np.abs(a - b).max() <= 1e-5


def _h2(x, scale=1.0):
    """x * scale as an f16 pair (hi, lo): hi = f16(x), lo = f16(x - hi), both returned as float64"""
    x = np.asarray(x, np.float32) * np.float32(scale)
    hi = x.astype(np.float16).astype(np.float32)
    lo = (x - hi).astype(np.float16).astype(np.float32)
    return hi.astype(np.float64), lo.astype(np.float64)


def test_f16_pair_arithmetic_is_f32_grade(golden_dir):
    """The default GPU kernels (csrc/k3_cnn_h2.hip) carry each f32 operand of conv2 and fc1 as an f16 pair hi + lo (weights
    pre-scaled by a power of two) and form a product as ah*wh + ah*wl + al*wh.  This simulates exactly that operand treatment
    (exact products, exact sums) on the golden inputs with the trained weights and checks the claim the kernel's header makes:
    its logits are as close to an exact (float64) evaluation of the model as PyTorch-CPU's own f32 forward is -- i.e. what the
    scheme gives up (operands cut to 22 bits, the lo*lo term) is below f32's own rounding noise, two orders inside the 1e-4
    contract."""
    import torch.nn.functional as F
    g = np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz"))
    sd = _coreml_sd(g)
    x = torch.from_numpy(cnn_oracle.golden_inputs(int(g["x_seed"]), 162))

    def head(feats64, mode):
        w1 = sd["fc1.weight"].numpy()
        if mode == "exact":
            h = feats64 @ torch.from_numpy(w1.astype(np.float64)).T
        else:
            e = 13 - int(np.floor(np.log2(np.abs(w1).max())))
            ah, al = _h2(feats64.numpy().astype(np.float32))
            wh, wl = _h2(w1, 2.0 ** e)
            h = (torch.from_numpy(ah) @ torch.from_numpy(wh).T + torch.from_numpy(ah) @ torch.from_numpy(wl).T
                 + torch.from_numpy(al) @ torch.from_numpy(wh).T) * 2.0 ** -e
        h = F.relu(h + sd["fc1.bias"].double()).float()
        return (h @ sd["fc2.weight"].T + sd["fc2.bias"]).numpy()

    with torch.no_grad():
        c1 = F.max_pool2d(F.relu(F.conv2d(x, sd["conv1.weight"], sd["conv1.bias"], padding=1)), 2, 2)      # f32, as the kernel
        w2 = sd["conv2.weight"].numpy()
        y_exact = F.conv2d(c1.double(), sd["conv2.weight"].double(), sd["conv2.bias"].double(), padding=1)
        e = 13 - int(np.floor(np.log2(np.abs(w2).max())))
        ah, al = (torch.from_numpy(t) for t in _h2(c1.numpy()))
        wh, wl = (torch.from_numpy(t) for t in _h2(w2, 2.0 ** e))
        y_pair = (F.conv2d(ah, wh, None, padding=1) + F.conv2d(ah, wl, None, padding=1) + F.conv2d(al, wh, None, padding=1)) * 2.0 ** -e
        y_pair = y_pair + sd["conv2.bias"].double().view(1, -1, 1, 1)
        f_exact = F.max_pool2d(F.relu(y_exact), 2, 2).reshape(162, -1)
        f_pair = F.max_pool2d(F.relu(y_pair), 2, 2).float().double().reshape(162, -1)                    # features are stored as f32
        exact = head(f_exact, "exact")
        pair = head(f_pair, "pair")
    torch_f32 = cnn_oracle.forward(sd, x).numpy()
    err_pair, err_torch = np.abs(pair - exact).max(), np.abs(torch_f32 - exact).max()
    assert err_pair <= 5e-6 and err_pair <= 2 * err_torch + 1e-7, (err_pair, err_torch)
    assert np.abs(pair - torch_f32).max() <= 1e-5
    assert (pair.argmax(1) == g["digits"]).all()


# ---- the float64 reference, the emulations and the tolerance rule of tests/test_gpu_cnn_accuracy.py --------------------------------
def _state(name, golden_dir):
    if name == "trained":
        return _coreml_sd(np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz")))
    return cnn_oracle.random_state_dict(1234)


def _cells(n, seed):
    rs = np.random.RandomState(seed)
    cells = rs.randint(0, 256, (n, 28, 28)).astype(np.uint8)
    cells[::3] = np.clip(cells[::3].astype(int) // 4 + 150, 0, 255).astype(np.uint8)    # ink-like cells beside the noise
    return cells


def test_forward64_reproduces_the_goldens(golden_dir):
    """forward64 lands on the goldens (captured from the reference's own f32 model) within PyTorch-CPU's own f32 distance from it."""
    for name, fx in (("random", "cnn_random_seed1234.npz"), ("trained", "cnn_coreml_fp16.npz")):
        g = np.load(os.path.join(golden_dir, fx))
        sd = _state(name, golden_dir)
        x = cnn_oracle.golden_inputs(int(g["x_seed"]), g["logits"].shape[0])
        want = cnn_oracle.forward64(sd, x).numpy()
        t32 = cnn_oracle.forward(sd, x).numpy()
        assert want.dtype == np.float64
        assert np.abs(want - g["logits"]).max() <= 2 * np.abs(t32 - want).max() + 1e-7, name
        assert (want.argmax(1) == g["digits"]).all()


@pytest.mark.parametrize("weights,mutation", [("random", m) for m in ("drop_al_wh", "drop_ah_wl", "conv2_bias", "drop_fc1_kstep")] +
                         [("trained", m) for m in ("drop_al_wh", "conv2_bias", "drop_fc1_kstep")])
def test_pair_tolerance_catches_mutations(golden_dir, weights, mutation):
    """The f32 families' rule, max|got - f64| <= C_F32 * max|torch_f32 - f64| + 2^-24 max|f64|: the exact emulation of the f16-pair kernels
    meets it with room to spare, and each injected bug breaks it.  (The trained weights are f16 values: their lo halves are all zero, so
    dropping ah*wl changes nothing there -- asserted in test_trained_weights_are_f16_values.)"""
    sd = _state(weights, golden_dir)
    x = cnn_oracle.glue(_cells(200, 3))
    want = cnn_oracle.forward64(sd, x).numpy()
    tol = cnn_oracle.tolerance(want, np.abs(cnn_oracle.forward(sd, x).numpy() - want).max(), cnn_oracle.C_F32)
    good = np.abs(cnn_oracle.forward_pair_emulated(sd, x).numpy() - want).max()
    assert good <= tol / 4, (good, tol)
    bad = np.abs(cnn_oracle.forward_pair_emulated(sd, x, mutate=mutation).numpy() - want).max()
    assert bad > tol, (mutation, bad, tol)


def test_trained_weights_are_f16_values(golden_dir):
    sd = _state("trained", golden_dir)
    for k in ("conv1.weight", "conv2.weight", "fc1.weight"):
        assert torch.equal(sd[k].half().float(), sd[k]), k


@pytest.mark.parametrize("mutation", ["truncate", "conv2_channel", "drop_fc1_kstep"])
@pytest.mark.parametrize("glue_mode", [0, 1])
def test_bf16_tolerance_catches_mutations(golden_dir, mutation, glue_mode):
    """The bf16 rule, max|got - emu64| <= C_BF16 * max|emu_f32acc - emu64| + 2^-24 max|emu64|, with the trained weights (what the bf16
    configuration serves): each injected bug breaks it; the emulation itself is within the bf16 scheme's distance of the f32 model."""
    sd = _state("trained", golden_dir)
    cells = _cells(300, 4)
    emu = cnn_oracle.forward_bf16_emulated(sd, cells, glue_mode).numpy()
    noise = np.abs(cnn_oracle.forward_bf16_emulated(sd, cells, glue_mode, acc=torch.float32).numpy() - emu).max()
    tol = cnn_oracle.tolerance(emu, noise, cnn_oracle.C_BF16)
    assert 0 < noise and tol < 3e-3, (noise, tol)
    assert np.abs(emu - cnn_oracle.forward64(sd, cnn_oracle.glue(cells, glue_mode)).numpy()).max() < 0.05
    bad = np.abs(cnn_oracle.forward_bf16_emulated(sd, cells, glue_mode, mutate=mutation).numpy() - emu).max()
    assert bad > tol, (mutation, bad, tol)


def test_glue_matches_the_oracle_glue():
    import sv_oracle
    cells = _cells(20, 5)
    assert np.array_equal(cnn_oracle.glue(cells), sv_oracle.cells_to_input(cells)[:, None])
    assert np.array_equal(cnn_oracle.glue(cells, 1), sv_oracle.cells_to_input(sv_oracle.preprocess_cells(cells))[:, None])


def test_fc1_weight_overflow_of_the_old_weight_scaling():
    """fc1.weight x 1e11: the loader used to floor the weight exponent at -14, so max|w| * 2^-14 (~1.1e5) overflowed f16 (hi = inf, lo = -inf)
    and the hidden units became NaN -- on the default kernels, since the range decision never looked at fc1.  (The emulation keeps the NaN;
    the kernels' ReLU, an IEEE maxNum, turned them into zeros, and the old build's logits were finite but wrong by 100 %: measured on an
    MI355X.)  The exponent now has no floor (any finite weight scales below 2^14): the emulation with the loader's present scaling is f32-grade."""
    sd = {k: v.clone() for k, v in cnn_oracle.random_state_dict(1234).items()}
    sd["fc1.weight"] *= 1e11
    x = cnn_oracle.glue(_cells(64, 6))
    assert cnn_oracle.pair_range(sd)["in_range"]                        # the default kernels take these weights
    old = cnn_oracle.forward_pair_emulated(sd, x, clamp=(-14, 40), act_scale=False).numpy()
    assert not np.isfinite(old).all()
    want = cnn_oracle.forward64(sd, x).numpy()
    got = cnn_oracle.forward_pair_emulated(sd, x).numpy()
    tol = cnn_oracle.tolerance(want, np.abs(cnn_oracle.forward(sd, x).numpy() - want).max(), cnn_oracle.C_F32)
    assert np.isfinite(got).all() and np.abs(got - want).max() <= tol


def test_tiny_activations_are_scaled_into_the_pairs_precision():
    """conv1 x 1e-11 (weights and bias) and conv2 x 2e9/max|w|: conv1's activations (~1e-11) are f16-subnormal or zero as unscaled pairs, so
    without the activation scale conv2 sees almost nothing; with it (eA ~ 37) the pairs keep their 22 bits."""
    sd = {k: v.clone() for k, v in cnn_oracle.random_state_dict(1234).items()}
    sd["conv1.weight"] *= 1e-11
    sd["conv1.bias"] *= 1e-11
    sd["conv2.weight"] *= 2e9 / float(sd["conv2.weight"].abs().max())
    r = cnn_oracle.pair_range(sd)
    assert r["in_range"] and r["eA"] > 30 and r["eF"] == 0
    x = cnn_oracle.glue(_cells(64, 7))
    want = cnn_oracle.forward64(sd, x).numpy()
    tol = cnn_oracle.tolerance(want, np.abs(cnn_oracle.forward(sd, x).numpy() - want).max(), cnn_oracle.C_F32)
    assert np.abs(cnn_oracle.forward_pair_emulated(sd, x).numpy() - want).max() <= tol
    unscaled = cnn_oracle.forward_pair_emulated(sd, x, act_scale=False).numpy()
    assert not np.isfinite(unscaled).all() or np.abs(unscaled - want).max() > 10 * tol


def test_pair_range_of_ordinary_weights_is_unscaled(golden_dir):
    """Trained and random weights keep eA = eF = 0: the activation scaling leaves the default kernels' arithmetic on them unchanged."""
    for name in ("trained", "random"):
        r = cnn_oracle.pair_range(_state(name, golden_dir))
        assert r["in_range"] and r["eA"] == 0 and r["eF"] == 0 and r["x_hi"] >= 1, (name, r)
