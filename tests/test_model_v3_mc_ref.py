"""CPU: the MC-dropout yardstick (tests/model_v3_mc_ref.py) and the host side of the feature -- the Philox4x32-10 mask generator against
its published known answers and against sv_mc_dropout_masks_host, the keep rates at a fixed seed, the masked restatement against
tests/model_v3_ref.py and against a golden the reference's own module produced (tests/golden/make_model_v3_mc_goldens.py), the module's
contract, and the mutation checks that show the bounds of tests/test_gpu_model_v3_mc.py catch plausible bugs."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import model_v3_mc_ref as mc
import model_v3_ref as ref
from cnn_oracle import tolerance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, OFFSET = 0x1234567887654321, 8


def _host():
    import sudoku_vision_amd as sva
    return sva.host


def test_philox_known_answers():
    """The Random123 known-answer vectors of philox4x32-10."""
    for counter, key, want in (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                               ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                               ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")):
        got = mc.philox4x32_10([np.uint32(c) for c in counter], key)
        assert " ".join(f"{int(v):08x}" for v in got) == want


@pytest.mark.parametrize("S,B", ((1, 1), (3, 2), (10, 81)))
@pytest.mark.parametrize("p_spatial,p_fc", ((0.0, 0.0), (0.1, 0.5), (0.5, 1.0), (0.1, 0.1)))
def test_host_generator_equals_the_numpy_restatement(S, B, p_spatial, p_fc):
    got = _host().mc_dropout_masks(SEED, OFFSET, S, B, p_spatial, p_fc)
    want = mc.masks(SEED, OFFSET, S, B, p_spatial, p_fc)
    for g, w, C in zip(got, want, mc.SITE_CHANNELS):
        assert g.shape == (S, B, C) and g.dtype == np.uint8 and np.array_equal(g, w)
    if p_spatial == 0:
        assert got[0].all() and got[1].all() and got[2].all()
    if p_fc == 1:
        assert not got[2].any()


def test_masks_are_a_pure_function_of_sample_and_cell():
    host = _host()
    big = host.mc_dropout_masks(SEED, OFFSET, 10, 81)
    for s, b in ((0, 0), (3, 50), (9, 80)):
        one = mc.masks(SEED, OFFSET, 1, 2, 0.1, 0.5, b0=b - 1 if b else 0, s0=s)      # B = 2, S = 1, shifted to (s, b)
        for g, w in zip(big, one):
            assert np.array_equal(g[s, b], w[0, 1 if b else 0])
    small = host.mc_dropout_masks(SEED, OFFSET, 4, 7)                                  # the same (s, b) at another B and S
    for g, w in zip(big, small):
        assert np.array_equal(g[:4, :7], w)
    for other in (host.mc_dropout_masks(SEED, OFFSET + 4, 10, 81), host.mc_dropout_masks(SEED + 1, OFFSET, 10, 81),
                  host.mc_dropout_masks(SEED, OFFSET + 2 ** 32, 10, 81), host.mc_dropout_masks(SEED + 2 ** 32, OFFSET, 10, 81)):
        assert all(not np.array_equal(g, w) and abs((g != w).mean() - 2 * g.mean() * (1 - g.mean())) < 0.02 for g, w in zip(big, other))
    with pytest.raises(ValueError):
        host.mc_dropout_masks(SEED, OFFSET, 0, 3)
    with pytest.raises(ValueError):
        host.mc_dropout_masks(SEED, OFFSET, 2, 3, p_spatial=1.0)
    with pytest.raises(ValueError):
        host.mc_dropout_masks(SEED, OFFSET, 2, 3, p_fc=1.5)


def test_keep_rates_at_a_fixed_seed():
    """S = 10, B = 81 at one seed: every share of kept bits is within 5 sigma of its rate, sigma = sqrt(p (1 - p) / count) -- overall
    (0.0078 for the 103,680 feature bits at 0.5, 0.0093 for layer1's 25,920 at 0.9), per channel and per sample.  The seed is fixed, so
    the test cannot flake; the numpy restatement is checked to be inside the bounds too."""
    for keep in (_host().mc_dropout_masks(SEED, OFFSET, 10, 81, 0.1, 0.5), mc.masks(SEED, OFFSET, 10, 81, 0.1, 0.5)):
        for k, rate in zip(keep, (0.9, 0.9, 0.5)):
            for what, share in (("all", k.mean()), ("channel", k.mean((0, 1))), ("sample", k.mean((1, 2)))):
                count = k.size / np.size(share)
                bound = 5 * np.sqrt(rate * (1 - rate) / count)
                print(f"keep share C={k.shape[2]} per {what}: worst {np.abs(share - rate).max():.4f}, 5 sigma {bound:.4f}")
                assert (np.abs(share - rate) <= bound).all(), (k.shape, what)
    assert abs(5 * np.sqrt(0.25 / 103680) - 0.0078) < 1e-4 and abs(5 * np.sqrt(0.09 / 25920) - 0.0093) < 1e-4


@pytest.mark.parametrize("use_se", (True, False))
def test_identity_masks_give_the_eval_forward(use_se):
    sd = ref.random_state_dict_v3(2024, use_se)
    x = ref.inputs(3, 5)
    ones = tuple(np.ones((5, c), np.uint8) for c in mc.SITE_CHANNELS)
    assert torch.equal(mc.forward64(sd, x, ones, 0.0, 0.0), ref.forward64(sd, x))
    assert torch.equal(mc.forward(sd, x, ones, 0.0, 0.0), ref.forward(sd, x))


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "model_v3_mc.npz"))
    sd = ref.random_state_dict_v3(int(g["w_seed"]), True)
    sd["temperature"] = torch.full((1,), float(g["temperature"]))
    x, keep = mc.expand(ref.inputs(int(g["x_seed"]), int(g["b"])), (g["keep1"], g["keep3"], g["keepf"]))
    return g, sd, x, keep


def test_restatement_reproduces_the_reference(golden_dir):
    """The rule of tests/test_model_v3_ref.py: the f32 restatement's error against float64 is no more than the reference module's own."""
    g, sd, x, keep = _golden(golden_dir)
    S, B, T = int(g["s"]), int(g["b"]), float(g["temperature"])
    p = (float(g["p_spatial"]), float(g["p_fc"]))
    assert 0 < keep[0].mean() < 1 and 0 < keep[1].mean() < 1 and 0 < keep[2].mean() < 1          # every site dropped something
    # one forward per sample, as the reference ran them: PyTorch-CPU's f32 convolution rounds differently at another batch size
    got = np.stack([mc.forward(sd, x[s * B:(s + 1) * B], tuple(k[s * B:(s + 1) * B] for k in keep), *p).numpy() for s in range(S)])
    want64 = mc.forward64(sd, x, keep, *p).numpy().reshape(S, B, 10)
    noise = np.abs(g["logits"].astype(np.float64) - want64).max()
    err = np.abs(got.astype(np.float64) - want64).max()
    print(f"mc logits: restatement err {err:.3e}, reference-module noise {noise:.3e}, bit-equal {np.array_equal(got, g['logits'])}")
    assert err <= tolerance(want64, noise, 1) and np.abs(got - g["logits"]).max() <= tolerance(want64, noise, 1)
    # the stacking code, on the reference's own logits: f32 in the reference, float64 here
    _, mean, std, predicted = mc.stats(g["logits"], T)
    assert np.abs(mean - g["mean"]).max() < 1e-6 and np.abs(std - g["std"]).max() < 1e-6 and np.array_equal(predicted, g["predicted"])


def test_new_symbols_are_exported_by_both_libraries():
    import sudoku_vision_amd as sva
    for handle in (sva._native.lib(), sva._native.lib_xcheck()):
        for n in ("sv_cnn3_forward_mc_f32", "sv_mc_dropout_masks_host"):
            assert hasattr(handle, n), n
        assert handle.sv_version() == 2


def test_module_contract(golden_dir):
    sys.path.insert(0, os.path.join(ROOT, "sudoku-vision_amd", "ml"))
    try:
        sys.modules.pop("model_v3", None)
        import model_v3
    finally:
        sys.path.pop(0)
    m = model_v3.DigitCNNv3()
    params = list(inspect.signature(m.forward_with_uncertainty).parameters.values())
    assert [(p.name, p.default) for p in params[:2]] == [("x", inspect.Parameter.empty), ("n_samples", 10)]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params[2:])
    x = torch.zeros(1, 1, 28, 28)
    with pytest.raises(ValueError):
        m.forward_with_uncertainty(x, n_samples=0)
    for attr, bad in (("spatial_dropout", 1.0), ("spatial_dropout", -0.1), ("dropout", 1.5)):
        old = getattr(m, attr).p
        getattr(m, attr).p = bad
        with pytest.raises(ValueError):
            m.forward_with_uncertainty(x)
        getattr(m, attr).p = old
    with pytest.raises(NotImplementedError):
        m.forward_with_uncertainty(x)                     # a CPU tensor: no fallback
    assert m.spatial_dropout.p == 0.1 and not list(m.spatial_dropout.parameters()) and not list(m.spatial_dropout.buffers())
    assert list(m.state_dict()) == [str(k) for k in np.load(os.path.join(golden_dir, "model_v3_se.npz"))["keys"]]
    assert not hasattr(model_v3.DigitCNNv3Light, "forward_with_uncertainty") and not hasattr(model_v3.EmptyClassifier, "forward_with_uncertainty")


@pytest.mark.parametrize("mutate", mc.MUTATIONS)
def test_bounds_catch_mutations(mutate):
    """Each plausible bug, applied to the float64 restatement, moves the result past the bound tests/test_gpu_model_v3_mc.py uses: the
    logits past C_V3 * noise + 2^-24 max|f64| for the two mask bugs, std or mean past their bounds for the two stacking bugs."""
    S, B, T = 4, 27, 2.5
    sd = ref.random_state_dict_v3(2024, True)
    keep3d = mc.masks(SEED, OFFSET, S, B, 0.1, 0.5)
    x, keep = mc.expand(ref.inputs(11, B), keep3d)
    want = mc.forward64(sd, x, keep, 0.1, 0.5).numpy()
    noise = np.abs(mc.forward(sd, x, keep, 0.1, 0.5).numpy().astype(np.float64) - want).max()
    tol = tolerance(want, noise, ref.C_V3)
    probs, mean, std, _ = mc.stats(want.reshape(S, B, 10), T)
    mean_bound, std_bound = mc.bounds(probs, mean, tol, T)
    if mutate in ("no_scale", "mask_per_pixel"):
        err = np.abs(mc.forward64(sd, x, keep, 0.1, 0.5, mutate=mutate).numpy() - want).max()
        print(f"{mutate}: moves the logits by {err:.3e}, tolerance {tol:.3e} (noise {noise:.3e})")
        assert err > tol
    else:
        _, mean_m, std_m, _ = mc.stats(want.reshape(S, B, 10), T, mutate=mutate)
        d_mean, d_std = np.abs(mean_m - mean), np.abs(std_m - std)
        print(f"{mutate}: moves mean by {d_mean.max():.3e} (bound {mean_bound.max():.3e}), std by {d_std.max():.3e} (bound {std_bound:.3e})")
        assert (d_std > std_bound).any() if mutate == "biased_std" else (d_mean > mean_bound).any()
