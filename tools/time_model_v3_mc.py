"""Timing of MC dropout on DigitCNNv3 (csrc/k8_cnn_v3.hip, Context.cnn3_forward_mc) at S = 10 samples of 81 and 81*16 cells.

    python tools/time_model_v3_mc.py [--iters 10] [--repeats 5] [--json out.json]

Per batch size, in windows that alternate (_timing.event_ms on a list): the MC entry; S calls of Context.cnn3_forward on the same batch,
the entry the parent commit has and the yardstick (by MAC count the MC entry does 0.22 + 0.78 S forwards' worth of matrix work, 0.80 of S
at S = 10); and PyTorch-ROCm running the reference-shaped loop (ml/model_v3.py:202-211: S forwards with the three dropouts drawn by
torch, softmax, stack, mean, std, argmax) on the drop-in's module structure evaluated with torch.nn.functional, BatchNorm on its
running statistics.  Needs a GPU; there is no CPU path."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sudoku_vision_amd as sva  # noqa: E402
from sudoku_vision_amd.runtime import _V3_BLOCKS  # noqa: E402
from _timing import cli, emit, event_ms  # noqa: E402
from time_model_v3 import random_state_dict  # noqa: E402

S, P_SPATIAL, P_FC = 10, 0.1, 0.5


def torch_mc(w, x):
    """forward_with_uncertainty's loop with torch's own dropout draws, on the device tensors w."""
    def bn(t, p):
        return F.batch_norm(t, w[p + ".running_mean"], w[p + ".running_var"], w[p + ".weight"], w[p + ".bias"], False, 0.0, 1e-5)

    def spatial(t):
        return t * torch.bernoulli(torch.ones(t.shape[0], t.shape[1], 1, 1, device=t.device) * (1 - P_SPATIAL)) / (1 - P_SPATIAL)

    probs = []
    for _ in range(S):
        t = F.relu(bn(F.conv2d(x, w["stem.0.weight"], None, 1, 1), "stem.1"))
        for i, (cin, c, stride) in enumerate(_V3_BLOCKS, 1):
            L = f"layer{i}"
            out = F.relu(bn(F.conv2d(t, w[L + ".conv1.weight"], None, stride, 1), L + ".bn1"))
            out = bn(F.conv2d(out, w[L + ".conv2.weight"], None, 1, 1), L + ".bn2")
            y = torch.sigmoid(F.linear(F.relu(F.linear(out.mean((2, 3)), w[L + ".se.excite.0.weight"])), w[L + ".se.excite.2.weight"]))
            out = out * y[:, :, None, None]
            sc = bn(F.conv2d(t, w[L + ".shortcut.0.weight"], None, stride, 0), L + ".shortcut.1") if (stride != 1 or cin != c) else t
            t = F.relu(out + sc)
            if i in (1, 3):
                t = spatial(t)
        logits = F.linear(F.dropout(t.mean((2, 3)), P_FC, True), w["fc.weight"], w["fc.bias"])
        probs.append(F.softmax(logits / w["temperature"], 1))
    stack = torch.stack(probs)
    mean = stack.mean(0)
    return mean, stack.std(0), mean.argmax(1)


def main():
    args = cli(__doc__, None, [("--iters", dict(type=int, default=10)), ("--repeats", dict(type=int, default=5))])
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    ctx = sva.default_context()
    sd = random_state_dict(1)
    ctx.load_state_dict_v3(sd)
    w = {k: v.cuda() for k, v in sd.items()}
    ctx.reserve(81 * 16)
    res = {"iters": args.iters, "repeats": args.repeats, "n_samples": S, "p_spatial": P_SPATIAL, "p_fc": P_FC, "sizes": {}}
    for frames in (1, 16):
        B = 81 * frames
        x = torch.from_numpy(np.random.RandomState(B).uniform(-1, 1, (B, 1, 28, 28)).astype(np.float32)).cuda()

        def plain():
            for _ in range(S):
                ctx.cnn3_forward(x)

        with torch.no_grad():
            mc, fwd, pt = event_ms([lambda: ctx.cnn3_forward_mc(x, S, P_SPATIAL, P_FC, 1, 0), plain, lambda: torch_mc(w, x)], args.iters, args.repeats, warmup=3)
        res["sizes"][str(B)] = {"cells": B, "mc_ms": mc.median, "mc_ms_min_max": [mc.min, mc.max], "s_plain_forwards_ms": fwd.median,
                                "s_plain_forwards_ms_min_max": [fwd.min, fwd.max], "mc_over_s_plain_forwards": mc.median / fwd.median,
                                "expected_by_mac_count": (0.22 + 0.78 * S) / S, "pytorch_rocm_loop_ms": pt.median, "pytorch_over_ours": pt.median / mc.median}
        print(f"B={B:5d} S={S}: cnn3_forward_mc {mc.median:8.4f} ms   {S} x cnn3_forward {fwd.median:8.4f} ms   ratio {mc.median / fwd.median:5.3f} "
              f"(by MAC count {(0.22 + 0.78 * S) / S:5.3f})   PyTorch-ROCm loop {pt.median:8.4f} ms ({pt.median / mc.median:5.2f}x)")
    emit(res, args.json)


if __name__ == "__main__":
    main()
