"""Times K21 (csrc/k21_eval.hip, Context.eval_metrics with read_back=False into preallocated stats) at 81, 1296, 20,736 and 1,048,576 cells:
HIP-event time of the call with every per-cell output, with none (aggregates only), and with a failure list of 100, next to
  - a device copy of the bytes the full call reads and writes (one pass over them),
  - those bytes / 8 TB/s,
  - the composed torch-ROCm path (softmax, argmax, bincount for the confusion matrix, bucketize + bincount for the bins),
  - the reference's numpy bookkeeping on the host (tests/eval_ref.py dataset_metrics, which restates ml/evaluate_v2.py:96-147) with its
    D2H copy of the logits, wall clock.
Medians over the windows with the spread (_timing.event_ms, wall_ms).  Speed is reported, not gated.

    python tools/time_eval.py [--json profiles/eval_time.json]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import eval_ref as er  # noqa: E402
import sudoku_vision_amd as sva  # noqa: E402
from _timing import cli, emit, event_ms, floor_ms, wall_ms  # noqa: E402

ALL = ("probs", "pred", "conf", "true_prob", "nll", "correct")


def stat(t):
    return {"median_ms": t.median, "min_ms": t.min, "max_ms": t.max}


def torch_path(z, labels, edges):
    p = torch.softmax(z, 1)
    conf, pred = p.max(1)
    ok = pred == labels
    cm = torch.bincount(labels * 10 + pred, minlength=100)
    b = torch.bucketize(conf.double(), edges, right=False) - 1          # edges[b] < conf <= edges[b + 1]
    b = b.clamp(0, 9)
    return cm, torch.bincount(b, minlength=10), torch.bincount(b, weights=ok.double(), minlength=10), torch.bincount(b, weights=conf.double(), minlength=10)


def host_path(z, labels):
    zh = z.cpu().numpy()
    r = er.per_cell(zh, labels)
    return er.dataset_metrics(r["p"].astype(np.float32), r["pred"], labels)


def main():
    args = cli(__doc__, 5)
    ctx = sva.default_context()
    edges = torch.linspace(0, 1, 11, dtype=torch.float64, device=ctx.device)
    rs = np.random.RandomState(0)
    res = {"rows": [], "iters": 20, "windows": args.windows, "warmup": 3}
    for B in (81, 1296, 20736, 1048576):
        zh = (rs.randn(B, 10) * 3).astype(np.float32)
        lh = np.where(rs.rand(B) < 0.9, zh.argmax(1), rs.randint(0, 10, B)).astype(np.int64)
        z, labels = torch.from_numpy(zh).to(ctx.device), torch.from_numpy(lh).to(ctx.device)
        stats = ctx.eval_stats_buffer()
        fails = torch.empty((100, 48), dtype=torch.uint8, device=ctx.device)
        nbytes = B * (40 + 8 + 40 + 1 + 4 + 4 + 4 + 1)
        src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device=ctx.device), torch.empty(nbytes // 2, dtype=torch.uint8, device=ctx.device)
        full, agg_only, with_list, copy, composed = event_ms([
            lambda: ctx.eval_metrics(z, labels, want=ALL, stats=stats, read_back=False),
            lambda: ctx.eval_metrics(z, labels, want=(), stats=stats, read_back=False),
            lambda: ctx.eval_metrics(z, labels, want=(), stats=stats, failures=fails, max_failures=100, read_back=False),
            lambda: dst.copy_(src),
            lambda: torch_path(z, labels, edges)], iters=res["iters"], windows=args.windows, warmup=res["warmup"])
        host = wall_ms(lambda: host_path(z, lh), runs=3, warmup=1)
        row = {"cells": B, "bytes_read_and_written": nbytes, "k21_all_outputs": stat(full), "k21_aggregates_only": stat(agg_only),
               "k21_aggregates_and_100_failures": stat(with_list), "device_copy_same_bytes": stat(copy), "hbm_floor_ms": floor_ms(nbytes),
               "torch_rocm_composed": stat(composed), "numpy_on_host_with_d2h": stat(host)}
        res["rows"].append(row)
        print(row, flush=True)
    res["note"] = ("k21 times include the host's allocation of the output tensors (torch.empty per wanted output) and three launches with a failure "
                   "list; the copy moves half the bytes in and half out")
    emit(res, args.json)


if __name__ == "__main__":
    main()
