"""CPU yardstick for the DigitCNNv3Light and EmptyClassifier forwards (sudoku-vision_amd/ml/model_v3.py, csrc/k12_cnn_v3_light.hip).
TEST INFRASTRUCTURE ONLY.

Restates the reference's ml/model_v3.py:232-320 in eval mode with plain torch.nn.functional calls on a state_dict-shaped mapping: conv,
batch_norm with the running statistics (NOT folded: folding is a choice of the kernels), ReLU, max_pool2d, mean, linear.  The model is
told from the keys ("classifier.1.weight": EmptyClassifier).  `forward` evaluates in f32, `forward64` in float64.  Pinned by
tests/golden/model_v3_light.npz and model_v3_empty.npz, which hold outputs of the reference's own modules
(tests/golden/make_model_v3_light_goldens.py); tests/test_model_v3_light_ref.py checks that.

`mutate` injects one plausible kernel bug, so that the tests can show the tolerance rule catches it:
  "no_eps"          BatchNorm's eps left out                                   (Light)
  "avg_pool"        average pooling in place of max                            (both)
  "pool_shift"      the pool windows start one pixel late (zero padded)        (both)
  "gap_count"       the global average divides by the bordered plane's 81      (Light)
  "no_conv_bias"    the conv biases dropped                                    (Empty)
  "flatten_hwc"     the flatten taken in (H, W, C) order                       (Empty)
  "no_hidden_relu"  the hidden layer's ReLU dropped                            (Empty)
"""
import numpy as np
import torch
import torch.nn.functional as F

from cnn_oracle import tolerance  # noqa: F401  (the rule the tests use, with the constants below)
from model_v3_ref import inputs  # noqa: F401  (the same seeded cells as the DigitCNNv3 tests)

MUTATIONS_LIGHT = ("no_eps", "avg_pool", "pool_shift", "gap_count")
MUTATIONS_EMPTY = ("avg_pool", "pool_shift", "no_conv_bias", "flatten_hwc", "no_hidden_relu")

# C of the tolerance rule  max|gpu - f64| <= C * max|torch_f32 - f64| + 2^-24 max|f64|:  about four times the largest ratio
# max|gpu - f64| / noise measured on an MI355X over tests/test_gpu_model_v3_light.py, rounded up to a power of two (that file's docstring
# and profiles/r12_model_v3_light_accuracy.txt have the measured ratios: 2.76 at the most for Light, 1.51 for Empty)
C_LIGHT = 16.0
C_EMPTY = 8.0

LIGHT_CONVS = ((0, 1, 24), (4, 24, 48), (8, 48, 96))


def layout_light():
    """(key, shape) of the float entries of a DigitCNNv3Light state_dict in key order (num_batches_tracked left out)."""
    out = [("temperature", (1,))]
    for i, cin, c in LIGHT_CONVS:
        out += [(f"features.{i}.weight", (c, cin, 3, 3))] + [(f"features.{i + 1}.{n}", (c,)) for n in ("weight", "bias", "running_mean", "running_var")]
    return out + [("fc.weight", (10, 96)), ("fc.bias", (10,))]


def layout_empty():
    """(key, shape) of an EmptyClassifier state_dict in key order."""
    return [("features.0.weight", (16, 1, 3, 3)), ("features.0.bias", (16,)), ("features.3.weight", (32, 16, 3, 3)), ("features.3.bias", (32,)),
            ("classifier.1.weight", (32, 1568)), ("classifier.1.bias", (32,)), ("classifier.4.weight", (1, 32)), ("classifier.4.bias", (1,))]


def random_state_dict_light(seed):
    """Deterministic weights from numpy's RandomState, drawn as model_v3_ref.random_state_dict_v3 draws them: BatchNorm gamma U(0.5, 1.5),
    beta N(0, 0.1), running mean N(0, 0.2), running variance log-uniform in [0.01, 2] (small enough that eps = 1e-5 shows); each conv He-scaled times sqrt(var) of its BN;
    fc N(0, 0.3) (96 features of mean ~0.4: logits spread over a few units)."""
    rs = np.random.RandomState(seed)
    sd = {}
    var = None
    for key, shape in reversed(layout_light()):          # reversed: a conv's BN variance is drawn before the conv itself
        name = key.rsplit(".", 1)[1] if key != "temperature" else key
        if key == "temperature":
            v = np.ones(1)
        elif name == "running_var":
            var = v = np.exp(rs.uniform(np.log(0.01), np.log(2.0), shape))
        elif name == "running_mean":
            v = rs.normal(0, 0.2, shape)
        elif key.startswith("fc"):
            v = rs.normal(0, 0.3, shape)
        elif name == "bias":
            v = rs.normal(0, 0.1, shape)
        elif len(shape) == 1:
            v = rs.uniform(0.5, 1.5, shape)
        else:
            v = rs.normal(0, np.sqrt(2.0 / np.prod(shape[1:])), shape) * np.sqrt(var)[:, None, None, None]
        sd[key] = torch.from_numpy(np.asarray(v, np.float32))
    return {k: sd[k] for k, _ in layout_light()}


def random_state_dict_empty(seed):
    """Deterministic EmptyClassifier weights: He-scaled convs and hidden layer, biases N(0, 0.1), output layer N(0, 1).  The output layer
    is then scaled and its bias set so that, over 128 of the seeded cells, the logit has spread 2 and median 1: the sigmoid then crosses
    both 0.5 and 0.9 inside the bulk of a batch."""
    rs = np.random.RandomState(seed)
    sd = {}
    for key, shape in layout_empty():
        if len(shape) == 1:
            v = rs.normal(0, 0.1, shape)
        else:
            v = rs.normal(0, 1.0 if key == "classifier.4.weight" else np.sqrt(2.0 / np.prod(shape[1:])), shape)
        sd[key] = torch.from_numpy(np.asarray(v, np.float32))
    sd["classifier.4.bias"][:] = 0.0
    z = _forward(sd, inputs(seed + 1, 128), torch.float64)[0].numpy()
    k = 2.0 / z.std()
    sd["classifier.4.weight"] *= float(k)
    sd["classifier.4.bias"][:] = float(1.0 - np.median(z) * k)
    return sd


def is_empty_model(sd):
    return "classifier.1.weight" in sd


def _pool(t, mutate):
    if mutate == "avg_pool":
        return F.avg_pool2d(t, 2, 2)
    if mutate == "pool_shift":
        return F.max_pool2d(F.pad(t[:, :, 1:, 1:], (0, 1, 0, 1)), 2, 2)
    return F.max_pool2d(t, 2, 2)


def _forward(sd, x, dtype, mutate=None):
    w = {k: torch.as_tensor(np.asarray(v.detach().cpu()) if isinstance(v, torch.Tensor) else np.asarray(v)).to(dtype)
         for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    x = torch.as_tensor(np.asarray(x), device="cpu").to(dtype)
    with torch.no_grad():
        if is_empty_model(w):
            assert mutate is None or mutate in MUTATIONS_EMPTY, mutate
            nb = mutate == "no_conv_bias"
            x = _pool(F.relu(F.conv2d(x, w["features.0.weight"], None if nb else w["features.0.bias"], 1, 1)), mutate)
            x = _pool(F.relu(F.conv2d(x, w["features.3.weight"], None if nb else w["features.3.bias"], 1, 1)), mutate)
            flat = x.permute(0, 2, 3, 1).flatten(1) if mutate == "flatten_hwc" else x.flatten(1)
            h = F.linear(flat, w["classifier.1.weight"], w["classifier.1.bias"])
            if mutate != "no_hidden_relu":
                h = F.relu(h)
            return F.linear(h, w["classifier.4.weight"], w["classifier.4.bias"]), flat
        assert mutate is None or mutate in MUTATIONS_LIGHT, mutate
        eps = 1e-30 if mutate == "no_eps" else 1e-5        # F.batch_norm refuses an eps of exactly 0
        for i, _, _ in LIGHT_CONVS:
            p = f"features.{i + 1}"
            x = F.conv2d(x, w[f"features.{i}.weight"], None, 1, 1)
            x = F.relu(F.batch_norm(x, w[p + ".running_mean"], w[p + ".running_var"], w[p + ".weight"], w[p + ".bias"], False, 0.0, eps))
            if i != 8:
                x = _pool(x, mutate)
        feat = x.sum((2, 3)) / 81.0 if mutate == "gap_count" else x.mean((2, 3))
        return F.linear(feat, w["fc.weight"], w["fc.bias"]), feat


def forward(sd, x, mutate=None, return_features=False):
    """x [B,1,28,28] -> DigitCNNv3Light: logits f32 [B,10] (CPU tensor), or (logits, features [B,96]); EmptyClassifier: the logit [B,1]."""
    lg, ft = _forward(sd, x, torch.float32, mutate)
    return (lg, ft) if return_features else lg


def forward64(sd, x, mutate=None, return_features=False):
    """forward() in float64, same op order."""
    lg, ft = _forward(sd, x, torch.float64, mutate)
    return (lg, ft) if return_features else lg
