"""CPU: the DigitCNNv3 yardstick (tests/model_v3_ref.py) against goldens captured from the reference's own ml/model_v3.py
(tests/golden/make_model_v3_goldens.py); the drop-in module's state_dict contract; the C ABI's additions; and the mutation checks that
show the tolerance rule of tests/test_gpu_model_v3.py catches plausible kernel bugs."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import model_v3_ref as ref
from cnn_oracle import tolerance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = (("se", True), ("nose", False))


def _golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"model_v3_{name}.npz"))


@pytest.mark.parametrize("name,use_se", VARIANTS)
def test_restatement_reproduces_the_reference(golden_dir, name, use_se):
    g = _golden(golden_dir, name)
    sd = ref.random_state_dict_v3(int(g["w_seed"]), use_se)
    x = ref.inputs(int(g["x_seed"]), int(g["n"]))
    lg, ft = ref.forward(sd, x, return_features=True)
    lg64, ft64 = ref.forward64(sd, x, return_features=True)
    for what, got, gold, want64 in (("logits", lg, g["logits"], lg64), ("features", ft, g["features"], ft64)):
        want64 = want64.numpy()
        noise = np.abs(gold.astype(np.float64) - want64).max()          # the reference module's own f32 error
        err = np.abs(got.numpy().astype(np.float64) - want64).max()
        print(f"{name} {what}: restatement err {err:.3e}, reference-module noise {noise:.3e}, bit-equal {np.array_equal(got.numpy(), gold)}")
        assert err <= tolerance(want64, noise, 1), (what, err, noise)
        assert np.abs(got.numpy() - gold).max() <= tolerance(want64, noise, 1)


@pytest.mark.parametrize("name,use_se", VARIANTS)
def test_dropin_module_has_the_reference_state_dict(golden_dir, name, use_se):
    """In a fresh interpreter with sudoku-vision_amd/ml on the path, `from model_v3 import DigitCNNv3` (pipeline/run_v2.py:101) resolves
    to an nn.Module whose state_dict has exactly the reference's keys, shapes and dtypes, in order."""
    g = _golden(golden_dir, name)
    code = (
        "import sys, json\n"
        f"sys.path.insert(0, {os.path.join(ROOT, 'sudoku-vision_amd', 'ml')!r})\n"
        "import torch\n"
        "from model_v3 import DigitCNNv3, count_parameters\n"
        f"m = DigitCNNv3(num_classes=10, dropout=0.5, use_se={use_se})\n"
        "assert isinstance(m, torch.nn.Module)\n"
        "sd = m.state_dict()\n"
        "print(json.dumps({'keys': list(sd), 'shapes': [','.join(map(str, v.shape)) for v in sd.values()],"
        " 'dtypes': [str(v.dtype) for v in sd.values()], 'n': count_parameters(m),"
        " 'floats': sum(v.numel() for v in sd.values() if v.dtype != torch.int64)}))\n")
    out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True).stdout
    import json
    got = json.loads(out.strip().splitlines()[-1])
    assert got["keys"] == [str(k) for k in g["keys"]]
    assert got["shapes"] == [str(s) for s in g["shapes"]]
    assert got["dtypes"] == [str(s) for s in g["dtypes"]]
    assert got["n"] == int(g["n_parameters"])
    # the header's float counts are what the module gives, and the runtime's blob layout is the float part of the key list
    header = open(os.path.join(ROOT, "include", "sudoku_vision_hip.h")).read()
    define = "SV_CNN3_PARAMS_SE" if use_se else "SV_CNN3_PARAMS_NOSE"
    assert int(re.search(rf"#define {define} (\d+)", header).group(1)) == got["floats"]
    floats = [(k, s) for k, s, d in zip(got["keys"], got["shapes"], got["dtypes"]) if d != "torch.int64"]
    assert [(k, ",".join(map(str, s))) for k, s in ref.layout(use_se)] == floats
    import sudoku_vision_amd as sva
    assert sva.runtime.v3_layout(use_se) == ref.layout(use_se)


def test_new_symbols_are_exported_by_both_libraries():
    import sudoku_vision_amd as sva
    names = ("sv_load_weights_v3_f32", "sv_cnn3_forward_f32", "sv_cnn3_forward_cells_u8", "sv_frames_to_digits_v3")
    for handle in (sva._native.lib(), sva._native.lib_xcheck()):
        for n in names:
            assert hasattr(handle, n), n
        assert handle.sv_version() == 2


def test_module_refuses_what_it_cannot_do():
    sys.path.insert(0, os.path.join(ROOT, "sudoku-vision_amd", "ml"))
    try:
        sys.modules.pop("model_v3", None)
        from model_v3 import DigitCNNv3
    finally:
        sys.path.pop(0)
    m = DigitCNNv3()
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 1, 28, 28))                       # training mode
    m.eval()
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 1, 28, 28))                       # CPU tensor
    with pytest.raises(NotImplementedError):
        m.forward_with_uncertainty(torch.zeros(1, 1, 28, 28))
    k0 = m._weights_key()
    m.set_temperature(1.5)
    k1 = m._weights_key()
    m.layer2.bn1.running_var.mul_(2.0)
    assert k0 != k1 != m._weights_key() and float(m.temperature) == 1.5


@pytest.mark.parametrize("mutate,use_se", [(m, se) for se in (True, False) for m in ref.MUTATIONS if se or m not in ("drop_se", "se_mean_count")])
def test_tolerance_catches_mutations(mutate, use_se):
    """Each plausible bug, applied to the float64 restatement (so that nothing but the bug separates it from the yardstick), moves the
    logits of one 81-cell batch by more than the bound the GPU test uses, C_V3 * noise + 2^-24 max|f64|."""
    sd = ref.random_state_dict_v3(2024, use_se)
    x = ref.inputs(11, 81)
    want = ref.forward64(sd, x).numpy()
    noise = np.abs(ref.forward(sd, x).numpy().astype(np.float64) - want).max()
    tol = tolerance(want, noise, ref.C_V3)
    err = np.abs(ref.forward64(sd, x, mutate=mutate).numpy() - want).max()
    print(f"{mutate} use_se={use_se}: moves the logits by {err:.3e}, tolerance {tol:.3e} (noise {noise:.3e})")
    assert err > tol, (mutate, err, tol)
