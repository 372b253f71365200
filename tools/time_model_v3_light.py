"""Timing of the DigitCNNv3Light and EmptyClassifier forwards (csrc/k12_cnn_v3_light.hip, Context.cnn3_light_forward / empty_forward) at 81,
81*16 and 81*256 cells.

    python tools/time_model_v3_light.py [--iters 20] [--repeats 5] [--json out.json]

Per batch size and model, in one process on one device: HIP-event time per call (_timing.event_ms: median of `repeats` windows of `iters` calls, after a
warm-up that also ramps the clock; the windows of the things compared alternate), the f32 matrix-pipe floor for the model's FLOP count
(8.47 MFLOP per cell for Light, 2.13 for Empty) both at the 155 TFLOP/s nominal peak and at the rate an 8192^3 f32 torch.matmul reaches
in this run, PyTorch-ROCm's own f32 eval forward of the same unfolded model written with torch.nn.functional, and cnn3_forward (K8) with
Light's speed-up over it.  Needs a GPU; there is no CPU path."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sudoku_vision_amd as sva  # noqa: E402
from sudoku_vision_amd.runtime import empty_layout, light_layout, v3_layout  # noqa: E402
from _timing import cli, emit, event_ms  # noqa: E402

F32_MATRIX_PEAK = 155e12
FLOP_PER_CELL = {"light": 8.47e6, "empty": 2.13e6}


def random_state_dict(layout, seed):
    """He-scaled convolutions, BatchNorm statistics near the identity: the timing does not depend on the values."""
    rs = np.random.RandomState(seed)
    sd = {}
    for key, shape in layout:
        leaf = key.rsplit(".", 1)[-1]
        bn_scale = leaf == "weight" and len(shape) == 1
        if key == "temperature" or leaf == "running_var" or bn_scale:
            v = rs.uniform(0.8, 1.2, shape)
        elif len(shape) == 1:
            v = rs.normal(0, 0.1, shape)
        else:
            v = rs.normal(0, np.sqrt(2.0 / np.prod(shape[1:])), shape)
        sd[key] = torch.from_numpy(v.astype(np.float32))
    return sd


def torch_light(w, x):
    """DigitCNNv3Light.forward in eval mode with torch.nn.functional on the device tensors w."""
    for i in (0, 4, 8):
        p = f"features.{i + 1}"
        x = F.conv2d(x, w[f"features.{i}.weight"], None, 1, 1)
        x = F.relu(F.batch_norm(x, w[p + ".running_mean"], w[p + ".running_var"], w[p + ".weight"], w[p + ".bias"], False, 0.0, 1e-5))
        if i != 8:
            x = F.max_pool2d(x, 2, 2)
    return F.linear(x.mean((2, 3)), w["fc.weight"], w["fc.bias"])


def torch_empty(w, x):
    """EmptyClassifier.forward in eval mode with torch.nn.functional."""
    x = F.max_pool2d(F.relu(F.conv2d(x, w["features.0.weight"], w["features.0.bias"], 1, 1)), 2, 2)
    x = F.max_pool2d(F.relu(F.conv2d(x, w["features.3.weight"], w["features.3.bias"], 1, 1)), 2, 2)
    return F.linear(F.relu(F.linear(x.flatten(1), w["classifier.1.weight"], w["classifier.1.bias"])), w["classifier.4.weight"], w["classifier.4.bias"])


def main():
    args = cli(__doc__, None, [("--iters", dict(type=int, default=20)), ("--repeats", dict(type=int, default=5))])
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    ctx = sva.default_context()
    sds = {"light": random_state_dict(light_layout(), 1), "empty": random_state_dict(empty_layout(), 2)}
    ctx.load_state_dict_v3_light(sds["light"])
    ctx.load_state_dict_empty(sds["empty"])
    ctx.load_state_dict_v3(random_state_dict(v3_layout(True), 3))
    ctx.reserve(81 * 256)
    w = {m: {k: v.cuda() for k, v in sd.items()} for m, sd in sds.items()}
    ours = {"light": ctx.cnn3_light_forward, "empty": ctx.empty_forward}
    theirs = {"light": torch_light, "empty": torch_empty}

    a = torch.randn(8192, 8192, device="cuda")
    b = torch.randn(8192, 8192, device="cuda")
    gemm_ms = event_ms(lambda: torch.matmul(a, b), 5, args.repeats, warmup=3).median
    gemm_rate = 2 * 8192 ** 3 / gemm_ms * 1e3
    del a, b
    print(f"f32 torch.matmul 8192^3: {gemm_ms:.3f} ms = {gemm_rate / 1e12:.1f} TFLOP/s (nominal f32 matrix peak {F32_MATRIX_PEAK / 1e12:.0f})")

    res = {"iters": args.iters, "repeats": args.repeats, "f32_matrix_peak_flops": F32_MATRIX_PEAK, "measured_f32_gemm_flops": gemm_rate,
           "flop_per_cell": FLOP_PER_CELL, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for frames in (1, 16, 256):
        B = 81 * frames
        x = torch.from_numpy(np.random.RandomState(B).uniform(-1, 1, (B, 1, 28, 28)).astype(np.float32)).cuda()
        iters = max(2, args.iters // (1 if frames < 256 else 4))
        row = {"cells": B}
        with torch.no_grad():
            k8_ms = None
            for m in ("light", "empty"):
                diff = float((ours[m](x) - theirs[m](w[m], x)).abs().max())
                fns = [lambda: ours[m](x), lambda: theirs[m](w[m], x)] + ([lambda: ctx.cnn3_forward(x)] if m == "light" else [])
                t = [r.median for r in event_ms(fns, iters, args.repeats, warmup=3)]      # the windows alternate between the functions
                ms, ms_torch = t[0], t[1]
                floor = B * FLOP_PER_CELL[m] / F32_MATRIX_PEAK * 1e3
                row[m] = {"ms": ms, "floor_ms_at_155TF": floor, "floor_ms_at_measured_gemm_rate": B * FLOP_PER_CELL[m] / gemm_rate * 1e3,
                          "fraction_of_f32_matrix_peak": floor / ms, "pytorch_rocm_f32_ms": ms_torch, "pytorch_over_ours": ms_torch / ms,
                          "max_abs_diff_vs_pytorch": diff}
                line = f"B={B:6d} {m:5s}: ours {ms:8.4f} ms ({100 * floor / ms:5.1f} % of 155 TF)  PyTorch-ROCm f32 {ms_torch:8.4f} ms  ratio {ms_torch / ms:5.2f}x  max|diff| {diff:.2e}"
                if m == "light":
                    k8_ms = t[2]
                    row[m]["k8_cnn3_forward_ms"] = k8_ms
                    row[m]["speedup_over_k8"] = k8_ms / ms
                    line += f"  K8 {k8_ms:8.4f} ms = {k8_ms / ms:5.1f}x"
                print(line, flush=True)
        res["sizes"][str(B)] = row
    emit(res, args.json)


if __name__ == "__main__":
    main()
