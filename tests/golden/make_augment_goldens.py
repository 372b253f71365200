#!/usr/bin/env python3
"""Writes tests/golden/augment_goldens.npz: what the reference's tools/augment_data.py itself draws and computes.

    python tests/golden/make_augment_goldens.py /path/to/reference/tools/augment_data.py

The reference module imports cv2, which is not available, so it is imported with a stand-in `cv2` module whose functions are the
numpy restatements of tests/augment_ref.py (and grid_v2_ref / warp_ref) and which records every call: name, matrices, sizes, border
mode.  The module's `random` is wrapped to record every draw, and its ten augmentation functions are wrapped to record their
arguments, input and output.  What is stored is therefore the reference's own draws, the matrices and sizes it hands to cv2, and its
own numpy arithmetic (adjust_brightness, adjust_contrast, random_erasing, the pad / crop of scale run for real); the outputs of the
cv2 calls are the restatement's.  Only recorded arrays are written; nothing of the reference's text.

Per chain c (one augment_image call):  c{c}_names  the functions applied, in order;  c{c}_params float64 [n, 9], c{c}_ints int64 [n, 5]
(see RECORD below);  c{c}_in / c{c}_out u8 [n, H, W] every function's input and output;  c{c}_draws float64, every value the call drew
from `random`, in order.  chains: int64 [n_chains, 4] = (seed, preset index, image index, n_augmentations).
The np.random steps (add_noise, elastic_transform) are pinned by their parameters only: their outputs here come from np.random and
are not what the GPU's Philox fields give."""
import importlib.util
import os
import random as _random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import augment_ref as ar  # noqa: E402
import warp_ref  # noqa: E402

PRESETS = ("light", "medium", "heavy")
SEEDS = (1, 2, 3, 4)
SHAPES = ((28, 28), (13, 17))
# what params / ints hold per function
RECORD = {
    "rotate": "params[:6] the matrix handed to warpAffine",
    "translate": "params[:6] the matrix handed to warpAffine, as float64",
    "perspective_warp": "params[:9] the matrix handed to warpPerspective",
    "adjust_brightness": "params[0] the uniform draw (delta = draw * 255)",
    "adjust_contrast": "params[0] the uniform draw (the factor)",
    "gaussian_blur": "ints[0] the kernel size handed to GaussianBlur",
    "add_noise": "params[0] the intensity argument",
    "elastic_transform": "params[0] alpha, params[1] the sigma handed to GaussianBlur; ints[0] = 1 if remap got BORDER_REPLICATE and INTER_LINEAR",
    "random_erasing": "nothing: the rectangle is pinned by in / out",
    "scale": "ints[0], ints[1] the (new_w, new_h) handed to resize",
}


class Cv2StandIn(types.ModuleType):
    BORDER_REPLICATE, BORDER_CONSTANT, INTER_LINEAR, IMREAD_GRAYSCALE = 1, 0, 1, 0

    def __init__(self):
        super().__init__("cv2")
        self.calls = []

    def getRotationMatrix2D(self, center, angle, scale):
        return ar.rotation_matrix(center, angle, scale)

    def warpAffine(self, image, matrix, dsize, borderMode=0):
        assert borderMode == self.BORDER_REPLICATE and dsize == (image.shape[1], image.shape[0])
        m = np.asarray(matrix, np.float64)
        self.calls.append(("warpAffine", m.reshape(-1)))
        return ar.warp_affine(image, m)

    def getPerspectiveTransform(self, src, dst):
        return ar.perspective_matrix(src, dst)

    def warpPerspective(self, image, matrix, dsize, borderMode=0):
        assert borderMode == self.BORDER_REPLICATE and dsize == (image.shape[1], image.shape[0])
        self.calls.append(("warpPerspective", np.asarray(matrix, np.float64).reshape(-1)))
        return ar.warp_perspective(image, matrix)

    def GaussianBlur(self, image, ksize, sigma):
        if image.dtype == np.uint8:
            assert ksize[0] == ksize[1] and sigma == 0
            self.calls.append(("GaussianBlur", np.array([ksize[0]], np.float64)))
            return ar.blur(image, ksize[0])
        assert image.dtype == np.float32 and tuple(ksize) == (0, 0)
        self.calls.append(("GaussianBlurF", np.array([sigma], np.float64)))
        return ar.field_blur(image, ar.elastic_taps(sigma)[1])

    def remap(self, image, map_x, map_y, interpolation, borderMode=0):
        self.calls.append(("remap", np.array([interpolation == self.INTER_LINEAR and borderMode == self.BORDER_REPLICATE], np.float64)))
        return ar.remap(image, map_x, map_y)

    def resize(self, image, dsize):
        self.calls.append(("resize", np.array(dsize, np.float64)))
        return warp_ref.resize(image, dsize)


class RandomRecorder:
    """The reference module's `random`: Python's global generator, every draw recorded."""

    def __init__(self):
        self.draws = []

    def _rec(self, v):
        self.draws.append(float(v))
        return v

    def uniform(self, a, b):
        return self._rec(_random.uniform(a, b))

    def random(self):
        return self._rec(_random.random())

    def randint(self, a, b):
        return self._rec(_random.randint(a, b))

    def choice(self, seq):
        return self._rec(_random.choice(seq))

    def sample(self, population, k):
        return _random.sample(population, k)

    def seed(self, s):
        _random.seed(s)


def load_reference(path):
    cv2 = Cv2StandIn()
    sys.modules["cv2"] = cv2
    spec = importlib.util.spec_from_file_location("reference_augment_data", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rec = RandomRecorder()
    mod.random = rec
    log = []

    def wrap(name):
        fn = getattr(mod, name)

        def wrapped(image, *args, **kwargs):
            c0, d0 = len(cv2.calls), len(rec.draws)
            out = fn(image, *args, **kwargs)
            log.append({"name": name, "args": args, "in": np.array(image), "out": np.array(out), "cv2": cv2.calls[c0:], "draws": rec.draws[d0:]})
            return out
        setattr(mod, name, wrapped)
    for name in RECORD:
        wrap(name)
    return mod, rec, log


def record_of(e):
    params, ints = np.zeros(9), np.zeros(5, np.int64)
    cv = dict(e["cv2"])
    name = e["name"]
    if name in ("rotate", "translate"):
        params[:6] = cv["warpAffine"]
    elif name == "perspective_warp":
        params[:9] = cv["warpPerspective"]
    elif name in ("adjust_brightness", "adjust_contrast"):
        params[0] = e["draws"][0]
    elif name == "gaussian_blur":
        ints[0] = int(cv["GaussianBlur"][0])
    elif name == "add_noise":
        params[0] = e["args"][1]
    elif name == "elastic_transform":
        params[0], params[1], ints[0] = e["args"][0], cv["GaussianBlurF"][0], int(cv["remap"][0])
    elif name == "scale":
        ints[:2] = cv["resize"].astype(np.int64)
    return params, ints


def main():
    mod, rec, log = load_reference(sys.argv[1])
    images = {f"image_{k}": ar.sample_image(h, w, seed=7 + k) for k, (h, w) in enumerate(SHAPES)}
    out = dict(images)
    chains = []
    jobs = [(s, p, k, 3) for s in SEEDS for p in range(3) for k in range(len(SHAPES))] + [(s, 2, k, 10) for s in (11, 12, 13) for k in range(len(SHAPES))]
    for c, (seed, p, k, n_aug) in enumerate(jobs):
        _random.seed(seed)
        np.random.seed(seed)
        del log[:]
        d0 = len(rec.draws)
        result = mod.augment_image(images[f"image_{k}"], mod.create_augmentation_pipeline(PRESETS[p]), n_aug)
        assert len(log) == n_aug and (result == log[-1]["out"]).all()
        recs = [record_of(e) for e in log]
        out[f"c{c}_names"] = np.array([e["name"] for e in log])
        out[f"c{c}_params"] = np.stack([r[0] for r in recs])
        out[f"c{c}_ints"] = np.stack([r[1] for r in recs])
        out[f"c{c}_in"] = np.stack([e["in"] for e in log])
        out[f"c{c}_out"] = np.stack([e["out"] for e in log])
        out[f"c{c}_draws"] = np.array(rec.draws[d0:], np.float64)
        chains.append((seed, p, k, n_aug))
    out["chains"] = np.array(chains, np.int64)
    out["presets"] = np.array(PRESETS)
    np.savez_compressed(os.path.join(HERE, "augment_goldens.npz"), **out)
    print(f"{len(chains)} chains written")


if __name__ == "__main__":
    main()
