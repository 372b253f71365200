import os, sys
sys.path[:0] = [os.getcwd(), os.path.join(os.getcwd(), "tools")]
import torch, sudoku_vision_amd as sva
from sudoku_vision_amd.synth import synth_frames
from _timing import event_ms
ctx = sva.default_context()
frames = synth_frames(256, 1080, 1920, seed=1, device="cuda")[0]
t = lambda fn: event_ms(fn, iters=30, windows=1, warmup=10).median
for n in (64, 128, 256):
    f = frames[:n]
    ob = torch.empty((n, 1080, 1920), dtype=torch.uint8, device="cuda")
    obits = torch.empty((n, 1080, 60), dtype=torch.int32, device="cuda")
    print(n, "bytes %.4f" % t(lambda: ctx.preprocess(f, out=ob)), "bits %.4f" % t(lambda: ctx.preprocess_bits(f, out=obits)),
          "despeckle_bits %.4f" % t(lambda: ctx.despeckle_bits(obits)))
