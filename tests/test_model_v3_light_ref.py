"""CPU: the DigitCNNv3Light / EmptyClassifier yardstick (tests/model_v3_light_ref.py) is the reference's models -- bit-equal to outputs of the
reference's own modules (tests/golden/model_v3_light.npz, model_v3_empty.npz) -- the tolerance rule of the GPU tests catches each injected
kernel bug, the drop-in modules keep the reference's state_dict, and calibrate_temperature is the optimisation the reference runs."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_oracle
import model_v3_light_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {"light": (ref.random_state_dict_light, ref.layout_light, ref.MUTATIONS_LIGHT, "C_LIGHT"),
          "empty": (ref.random_state_dict_empty, ref.layout_empty, ref.MUTATIONS_EMPTY, "C_EMPTY")}


def _golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", f"model_v3_{name}.npz"))


@pytest.mark.parametrize("name", ("light", "empty"))
def test_restatement_is_the_reference_model(name):
    g = _golden(name)
    sd = MODELS[name][0](int(g["w_seed"]))
    x = ref.inputs(int(g["x_seed"]), int(g["n"]))
    out = ref.forward(sd, x).numpy()
    assert out.shape == g["logits"].shape and np.array_equal(out, g["logits"])
    float_keys = [k for k in g["keys"] if not k.endswith("num_batches_tracked")]
    assert float_keys == [k for k, _ in MODELS[name][1]()]
    assert sum(int(np.prod(s)) for _, s in MODELS[name][1]()) == {"light": 53699, "empty": 55041}[name]     # the C ABI's blob sizes


@pytest.mark.parametrize("name", ("light", "empty"))
def test_tolerance_rule_catches_each_mutation(name):
    make, _, mutations, cname = MODELS[name]
    sd = make(2024)
    x = ref.inputs(5, 81)
    want = ref.forward64(sd, x).numpy()
    noise = float(np.abs(ref.forward(sd, x).numpy() - want).max())
    tol = cnn_oracle.tolerance(want, noise, getattr(ref, cname))
    for m in mutations:
        err = float(np.abs(ref.forward64(sd, x, mutate=m).numpy() - want).max())
        print(f"MUT {name} {m}: err {err:.3e} = {err / tol:.1f} x the GPU bound {tol:.3e}")
        assert err > 10 * tol, (name, m, err, tol)


def _dropin():
    sys.path.insert(0, os.path.join(ROOT, "sudoku-vision_amd", "ml"))
    try:
        import model_v3
    finally:
        sys.path.pop(0)
    return model_v3


@pytest.mark.parametrize("name", ("light", "empty"))
def test_dropin_modules_keep_the_reference_state_dict(name):
    model_v3 = _dropin()
    g = _golden(name)
    m = model_v3.DigitCNNv3Light() if name == "light" else model_v3.EmptyClassifier()
    full = m.state_dict()
    assert list(full) == list(g["keys"])
    assert [",".join(map(str, v.shape)) for v in full.values()] == list(g["shapes"])
    assert [str(v.dtype) for v in full.values()] == list(g["dtypes"])
    assert model_v3.count_parameters(m) == int(g["n_parameters"])
    sd = MODELS[name][0](2024)
    m.load_state_dict({**{k: v for k, v in full.items() if k.endswith("num_batches_tracked")}, **sd}, strict=True)
    if name == "light":
        assert m.temperature.requires_grad is False and hasattr(m, "get_confidence")
        assert model_v3.DigitCNNv3Light(num_classes=10, dropout=0.3).dropout.p == 0.3
    else:
        assert hasattr(m, "is_empty")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval()(torch.zeros(1, 1, 28, 28))


def test_runtime_layouts_are_the_state_dict_order():
    import sudoku_vision_amd as sva
    assert sva.runtime.light_layout() == ref.layout_light()
    assert sva.runtime.empty_layout() == ref.layout_empty()


class _Stub(torch.nn.Module):
    """Returns fixed logits for the rows asked for: data is a column of row indices."""

    def __init__(self, logits):
        super().__init__()
        self.logits = logits
        self.calls = 0

    def forward(self, idx):
        self.calls += 1
        return self.logits[idx]


def test_calibrate_temperature_is_the_reference_procedure(capsys):
    model_v3 = _dropin()
    rs = np.random.RandomState(3)
    n = 600
    labels = torch.from_numpy(rs.randint(0, 10, n))
    clean = torch.from_numpy(rs.normal(0, 1, (n, 10)))
    clean[torch.arange(n), labels] += 2.0
    wrong = torch.from_numpy(rs.rand(n) < 0.25)                       # an over-confident model: logits scaled up, a quarter of them wrong
    clean[wrong] = clean[wrong].roll(1, 1)
    logits = (clean * 4.0).float()
    loader = [(torch.arange(i, min(i + 128, n)), labels[i:i + 128]) for i in range(0, n, 128)]
    stub = _Stub(logits)
    got = model_v3.calibrate_temperature(stub, loader, torch.device("cpu"))
    assert stub.calls == len(loader) and not stub.training
    # the procedure, written out: LBFGS(lr 0.01, max_iter 50) on cross_entropy(logits / T, labels) from T = 1.5, one step
    t = torch.nn.Parameter(torch.ones(1) * 1.5)
    opt = torch.optim.LBFGS([t], lr=0.01, max_iter=50)

    def closure():
        opt.zero_grad()
        loss = F.cross_entropy(logits / t, labels)
        loss.backward()
        return loss

    opt.step(closure)
    assert isinstance(got, float) and abs(got - t.item()) <= 1e-6
    assert F.cross_entropy(logits / got, labels) < F.cross_entropy(logits, labels)
    assert "Calibrated temperature" in capsys.readouterr().out
    # other arguments reach the optimiser
    t2 = torch.nn.Parameter(torch.ones(1) * 1.5)
    opt2 = torch.optim.LBFGS([t2], lr=0.1, max_iter=5)

    def closure2():
        opt2.zero_grad()
        loss = F.cross_entropy(logits / t2, labels)
        loss.backward()
        return loss

    opt2.step(closure2)
    assert abs(model_v3.calibrate_temperature(stub, loader, torch.device("cpu"), lr=0.1, max_iter=5) - t2.item()) <= 1e-6
    assert abs(t2.item() - t.item()) > 1e-3


def test_seeds_of_the_gpu_tests_meet_the_gap_caps():
    """tests/test_gpu_model_v3_light.py asserts that at most 1 % of a batch's cells fall under the top-2 gap (digits) or next to the
    threshold (is_empty).  Here the reference alone is shown to meet both caps for that file's seeds, with the bound those tests use."""
    for w_seed, x_seed, n in ((2024, 5, 2000), (2024, 5, 81), (77, 9, 81)):
        x = ref.inputs(x_seed, n)
        sd = ref.random_state_dict_light(w_seed)
        want = ref.forward64(sd, x).numpy()
        tol = cnn_oracle.tolerance(want, float(np.abs(ref.forward(sd, x).numpy() - want).max()), ref.C_LIGHT)
        top2 = np.sort(want, 1)[:, -2:]
        assert (top2[:, 1] - top2[:, 0] <= 2 * tol).sum() <= 0.01 * n
        sd = ref.random_state_dict_empty(w_seed)
        want = ref.forward64(sd, x).numpy()
        tol = cnn_oracle.tolerance(want, float(np.abs(ref.forward(sd, x).numpy() - want).max()), ref.C_EMPTY)
        p = 1.0 / (1.0 + np.exp(-want))
        for thr in (0.5, 0.9):
            assert (np.abs(p - thr) <= 0.25 * tol + 1e-7).sum() <= 0.01 * n       # |d sigmoid / dz| <= 1/4
            assert 0.05 * n < (p < thr).sum() < 0.95 * n                           # both decisions occur
