"""CPU yardstick for MC dropout on DigitCNNv3 (DigitCNNv3.forward_with_uncertainty, sv_cnn3_forward_mc_f32).  TEST INFRASTRUCTURE ONLY.

Three independent restatements:
  * Philox4x32-10 and the keep rule of include/sudoku_vision_hip.h in numpy (`philox4x32_10`, `masks`), sharing no code with csrc/sv_philox.h;
  * the forward of tests/model_v3_ref.py with the three dropouts of the reference's ml/model_v3.py:163-184 as explicit keep-mask arguments
    (`forward`, `forward64`): x * keep / (1 - p) per channel after layer1 and layer3 (:80-92), F.dropout's keep / (1 - p) on the pooled
    features, BatchNorm on its running statistics;
  * the stacking code of forward_with_uncertainty (:205-211) in float64 (`stats`).
Pinned by tests/golden/model_v3_mc.npz, which the reference's own module produced (tests/golden/make_model_v3_mc_goldens.py).

`mutate` injects one plausible bug:  "no_scale" layer3's kept channels are not scaled by 1 / (1 - p);  "mask_per_pixel" layer1's mask
is applied per pixel, not per channel;  "biased_std" divides by S;  "softmax_before_temperature" divides softmax(logits) by T."""
import numpy as np
import torch
import torch.nn.functional as F

import model_v3_ref as ref

MUTATIONS = ("no_scale", "mask_per_pixel", "biased_std", "softmax_before_temperature")
SITE_CHANNELS = (32, 64, 128)
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcast together), key: two uint32 scalars -> four uint32 arrays."""
    c = [np.asarray(v, np.uint64) & np.uint64(0xFFFFFFFF) for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    lo32, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & lo32, (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & lo32]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def keep_threshold(p):
    return int(np.rint((1.0 - np.float64(np.float32(p))) * 4294967296.0))


def masks(seed, offset, S, B, p_spatial, p_fc, b0=0, s0=0):
    """(keep1 u8 [S,B,32], keep3 [S,B,64], keepf [S,B,128]) of samples s0 .. s0+S-1 of cells b0 .. b0+B-1."""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    out = []
    for site, C in enumerate(SITE_CHANNELS):
        s = (np.arange(S, dtype=np.uint64) + np.uint64(s0))[:, None, None]
        b = (np.arange(B, dtype=np.uint64) + np.uint64(b0))[None, :, None]
        g = np.arange(C // 4, dtype=np.uint64)[None, None, :]
        c2 = np.uint64(site * 64) + g + np.uint64(((offset >> 32) & 0xFFFFFF) << 8)
        words = philox4x32_10((b, s, c2, np.uint64(offset & 0xFFFFFFFF)), (seed & 0xFFFFFFFF, seed >> 32))
        w = np.stack(words, -1).reshape(S, B, C).astype(np.uint64)
        out.append((w < np.uint64(keep_threshold(p_fc if site == 2 else p_spatial))).astype(np.uint8))
    return tuple(out)


def _forward(sd, x, keep, p_spatial, p_fc, dtype, mutate=None):
    """x [N,1,28,28] (N = every (sample, cell) row), keep = (keep1 [N,32], keep3 [N,64], keepf [N,128]) -> logits [N,10]."""
    assert mutate is None or mutate in MUTATIONS, mutate
    w = {k: torch.as_tensor(np.asarray(v.detach().cpu()) if isinstance(v, torch.Tensor) else np.asarray(v)).to(dtype)
         for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    use_se = any(".se.excite." in k for k in w)
    k1, k3, kf = (torch.as_tensor(np.asarray(k)).to(dtype) for k in keep)

    def bn(t, p):
        return F.batch_norm(t, w[p + ".running_mean"], w[p + ".running_var"], w[p + ".weight"], w[p + ".bias"], False, 0.0, 1e-5)

    def spatial(t, k, layer):
        m = k[:, :, None, None]
        if mutate == "mask_per_pixel" and layer == 1:         # pixel i of channel c takes channel (c + i) % C's bit
            C, hw = t.shape[1], t.shape[2] * t.shape[3]
            idx = (torch.arange(C)[:, None] + torch.arange(hw)[None, :]) % C
            m = k[:, idx].reshape(t.shape)
        if mutate == "no_scale" and layer == 3:
            return t * m
        return t * m / (1 - p_spatial)

    x = torch.as_tensor(np.asarray(x), device="cpu").to(dtype)
    with torch.no_grad():
        x = F.relu(bn(F.conv2d(x, w["stem.0.weight"], None, 1, 1), "stem.1"))
        for i, (cin, c, stride) in enumerate(ref.BLOCKS, 1):
            L = f"layer{i}"
            out = F.relu(bn(F.conv2d(x, w[L + ".conv1.weight"], None, stride, 1), L + ".bn1"))
            out = bn(F.conv2d(out, w[L + ".conv2.weight"], None, 1, 1), L + ".bn2")
            if use_se:
                y = torch.sigmoid(F.linear(F.relu(F.linear(out.mean((2, 3)), w[L + ".se.excite.0.weight"])), w[L + ".se.excite.2.weight"]))
                out = out * y[:, :, None, None]
            sc = x
            if stride != 1 or cin != c:
                sc = bn(F.conv2d(x, w[L + ".shortcut.0.weight"], None, stride, 0), L + ".shortcut.1")
            x = F.relu(out + sc)
            if i in (1, 3):
                x = spatial(x, k1 if i == 1 else k3, i)
        feat = x.mean((2, 3))
        feat = feat * kf / (1 - p_fc) if p_fc < 1 else feat * 0
        return F.linear(feat, w["fc.weight"], w["fc.bias"])


def forward(sd, x, keep, p_spatial, p_fc, mutate=None):
    return _forward(sd, x, keep, p_spatial, p_fc, torch.float32, mutate)


def forward64(sd, x, keep, p_spatial, p_fc, mutate=None):
    return _forward(sd, x, keep, p_spatial, p_fc, torch.float64, mutate)


def expand(x, keep):
    """x [B,...], keep three [S,B,C] -> (x repeated per sample [S*B,...], keep as [S*B,C]): row s*B + b."""
    S = keep[0].shape[0]
    return np.concatenate([x] * S), tuple(k.reshape(-1, k.shape[-1]) for k in keep)


def stats(logits, temperature=1.0, mutate=None):
    """logits [S,B,10] -> (probs [S,B,10], mean [B,10], std [B,10], predicted [B]) in float64, the reference's :205-211."""
    lg = torch.as_tensor(np.asarray(logits)).double()
    probs = F.softmax(lg, 2) / temperature if mutate == "softmax_before_temperature" else F.softmax(lg / temperature, 2)
    mean = probs.mean(0)
    std = probs.std(0, unbiased=mutate != "biased_std") if probs.shape[0] > 1 or mutate == "biased_std" else torch.full_like(mean, float("nan"))
    return probs.numpy(), mean.numpy(), std.numpy(), mean.argmax(1).numpy()


def bounds(probs64, mean64, tol, temperature):
    """The GPU tests' bounds for mean and std, from the logit tolerance `tol` carried through the softmax as tests/test_gpu_model_v3.py
    carries it for conf: |dp| <= p expm1(2 tol / |T|) + 2e-6 per sample; centring is a projection, so a perturbation of at most e per
    sample moves the centred vector's norm by at most sqrt(S) e: |dstd| <= sqrt(S / (S - 1)) e + 2e-6, e the largest per-sample bound."""
    S = probs64.shape[0]
    t = np.expm1(min(2 * tol / abs(temperature), 50.0))
    e = float((probs64 * t).max())
    return mean64 * t + 2e-6, (np.sqrt(S / (S - 1.0)) * e if S > 1 else 0.0) + 2e-6
