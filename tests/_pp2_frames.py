"""1080p test frames for cv/preprocess_v2.py: synth_frames with integer noise, with and without a painted shadow gradient and
a glare patch, built so that has_shadow and has_glare each take both values (the restatement decides; the tests assert it)."""
import numpy as np


def variants(frames):
    """frames u8 [>=2,H,W,3] (numpy, from synth_frames) -> list of (name, BGR u8 [H,W,3])."""
    rs = np.random.RandomState(5)
    H, W = frames.shape[1:3]
    # low contrast: the printed digits stay within 30 gray levels of the paper, so nothing reads as shadow
    flat = (frames[0] // 8 + 150 + rs.randint(0, 8, frames[0].shape)).astype(np.uint8)
    shadow = flat.astype(np.int32)
    ramp = np.linspace(30, 60, H).astype(np.int32)[:, None, None]          # a gradient, darker at the top
    for x0 in range(W // 12, W - 60, W // 6):                               # six 40-px bands
        shadow[:, x0:x0 + 40] = shadow[:, x0:x0 + 40] * ramp // 100
    shadow = shadow.astype(np.uint8)
    glare = frames[1].copy()
    glare[H // 10:H // 10 + H // 4, W // 8:W // 8 + W // 5] = 255
    both = shadow.copy()
    both[H // 2:H // 2 + H // 5, W // 2:W // 2 + W // 5] = 254
    return [("flat", flat), ("shadow", shadow), ("synth_glare", glare), ("shadow_glare", both)]
