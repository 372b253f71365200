"""Timing of the DigitCNNv3 forward (csrc/k8_cnn_v3.hip, Context.cnn3_forward) at 81, 81*16 and 81*256 cells.

    python tools/time_model_v3.py [--iters 20] [--repeats 5] [--json out.json]

Per batch size: HIP-event time per call (_timing.event_ms: median of `repeats` windows of `iters` calls, after a warm-up that also ramps the clock), the
fraction of the 155 TFLOP/s f32 matrix peak that time amounts to (132.5 MFLOP per cell), and, in the same process, PyTorch-ROCm's own
f32 eval forward of the same weights: the drop-in's module structure evaluated with torch.nn.functional (conv2d, batch_norm with
running statistics, ...) on the device.  Needs a GPU; there is no CPU path."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sudoku_vision_amd as sva  # noqa: E402
from sudoku_vision_amd.runtime import _V3_BLOCKS, v3_layout  # noqa: E402
from _timing import cli, emit, event_ms  # noqa: E402

F32_MATRIX_PEAK = 155e12
FLOP_PER_CELL = 132.5e6


def random_state_dict(seed):
    """He-scaled convolutions, BatchNorm statistics near the identity, small gates: the timing does not depend on the values."""
    rs = np.random.RandomState(seed)
    sd = {}
    for key, shape in v3_layout(True):
        leaf = key.rsplit(".", 1)[-1]
        if key == "temperature" or leaf == "running_var" or (leaf == "weight" and len(shape) == 1):
            v = rs.uniform(0.8, 1.2, shape)
        elif len(shape) == 1:
            v = rs.normal(0, 0.1, shape)
        else:
            v = rs.normal(0, np.sqrt(2.0 / np.prod(shape[1:])), shape)
        sd[key] = torch.from_numpy(v.astype(np.float32))
    return sd


def torch_forward(w, x):
    """DigitCNNv3.forward in eval mode with torch.nn.functional on the device tensors w."""
    def bn(t, p):
        return F.batch_norm(t, w[p + ".running_mean"], w[p + ".running_var"], w[p + ".weight"], w[p + ".bias"], False, 0.0, 1e-5)
    x = F.relu(bn(F.conv2d(x, w["stem.0.weight"], None, 1, 1), "stem.1"))
    for i, (cin, c, stride) in enumerate(_V3_BLOCKS, 1):
        L = f"layer{i}"
        out = F.relu(bn(F.conv2d(x, w[L + ".conv1.weight"], None, stride, 1), L + ".bn1"))
        out = bn(F.conv2d(out, w[L + ".conv2.weight"], None, 1, 1), L + ".bn2")
        y = torch.sigmoid(F.linear(F.relu(F.linear(out.mean((2, 3)), w[L + ".se.excite.0.weight"])), w[L + ".se.excite.2.weight"]))
        out = out * y[:, :, None, None]
        sc = bn(F.conv2d(x, w[L + ".shortcut.0.weight"], None, stride, 0), L + ".shortcut.1") if (stride != 1 or cin != c) else x
        x = F.relu(out + sc)
    return F.linear(x.mean((2, 3)), w["fc.weight"], w["fc.bias"])


def main():
    args = cli(__doc__, None, [("--iters", dict(type=int, default=20)), ("--repeats", dict(type=int, default=5))])
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    ctx = sva.default_context()
    sd = random_state_dict(1)
    ctx.load_state_dict_v3(sd)
    w = {k: v.cuda() for k, v in sd.items()}
    ctx.reserve(81 * 256)
    res = {"iters": args.iters, "repeats": args.repeats, "f32_matrix_peak_flops": F32_MATRIX_PEAK, "flop_per_cell": FLOP_PER_CELL, "sizes": {}}
    for frames in (1, 16, 256):
        B = 81 * frames
        x = torch.from_numpy(np.random.RandomState(B).uniform(-1, 1, (B, 1, 28, 28)).astype(np.float32)).cuda()
        iters = max(2, args.iters // (1 if frames < 256 else 4))
        with torch.no_grad():
            diff = float((ctx.cnn3_forward(x) - torch_forward(w, x)).abs().max())
            ms = event_ms(lambda: ctx.cnn3_forward(x), iters, args.repeats, warmup=3).median
            ms_torch = event_ms(lambda: torch_forward(w, x), iters, args.repeats, warmup=3).median
        floor = B * FLOP_PER_CELL / F32_MATRIX_PEAK * 1e3
        res["sizes"][str(B)] = {"cells": B, "ms": ms, "floor_ms_at_155TF": floor, "fraction_of_f32_matrix_peak": floor / ms,
                                "tflops": B * FLOP_PER_CELL / ms / 1e9, "pytorch_rocm_f32_ms": ms_torch, "pytorch_over_ours": ms_torch / ms,
                                "max_abs_diff_vs_pytorch": diff}
        print(f"B={B:6d}: cnn3_forward {ms:9.4f} ms  ({100 * floor / ms:5.1f} % of 155 TF)   PyTorch-ROCm f32 {ms_torch:9.4f} ms   ratio {ms_torch / ms:5.2f}x   max|diff| {diff:.2e}")
    emit(res, args.json)


if __name__ == "__main__":
    main()
