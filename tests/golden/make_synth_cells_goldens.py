#!/usr/bin/env python3
"""Writes tests/golden/synth_cells_goldens.npz: what the reference's ml/generate_synthetic_v2.py itself draws and computes.

    python tests/golden/make_synth_cells_goldens.py /path/to/reference/ml/generate_synthetic_v2.py /path/to/a/font.ttf

The reference module imports cv2, which is not available, so it is imported with a stand-in `cv2` whose functions are the numpy
restatements of tests/synth_cells_ref.py / augment_ref.py and which records every call with its arguments, input and output.  The
module's `random` is wrapped to record every draw and its `np.random.normal` to record its parameters.  Pillow is real, with the font
given on the command line.  What is stored is therefore the reference's own draws, its own numpy and Pillow arithmetic (plain and
gradient backgrounds, grain, artefacts, smudge, the glyph blend, brightness, contrast, pad / crop), the parameters it hands to cv2 and
to np.random, and -- from the restatement -- the outputs of the cv2 calls.  The outputs of the np.random fields are NumPy's and are not
what the GPU's Philox fields give: they are pinned by their parameters only.  Only recorded arrays are written; nothing of the
reference's text.

Per cell c (one pass of generate_dataset's loop body):
  cells int64 [n, 6] = (seed, label, size, font size or 0, 1 if no np.random field was drawn: the whole output is comparable,
                    the number of np.random.normal calls the base image made)
  c{c}_draws float64: every value drawn from `random`, in order;  c{c}_next: the next random.random() after the cell
  c{c}_base u8: generate_digit's / generate_empty_cell's output;  c{c}_out u8: apply_augmentation's output
  c{c}_bg u8: generate_paper_background's output;  c{c}_art_in / c{c}_art_out: add_grid_artifacts' (when called)
  c{c}_normal float64 [k, 1]: the sigma of every np.random.normal call, in order
  c{c}_cv_names, c{c}_cv_params float64 [k, 10], c{c}_cv_in / c{c}_cv_out u8 [k, S, S]: every cv2 call that takes an image (RECORD below)
  c{c}_mask u8, c{c}_glyph int64 [6] = (off_x, off_y, bbox): the glyph of a digit cell, so that no test needs the font."""
import importlib.util
import os
import random as _random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import augment_ref as ar  # noqa: E402
import synth_cells_ref as sr  # noqa: E402
import warp_ref  # noqa: E402

RECORD = {
    "warpAffine": "params[:6] the matrix, params[6] borderValue",
    "warpPerspective": "params[:9] the matrix, params[9] borderValue",
    "resize": "params[:2] dsize",
    "copyMakeBorder": "params[:4] top, bottom, left, right, params[4] value",
    "GaussianBlur": "params[0] ksize, params[1] sigma",
    "erode": "nothing (a 2 x 2 kernel of ones is asserted)",
    "dilate": "nothing (a 2 x 2 kernel of ones is asserted)",
}
JOBS = [(seed, label, 28) for seed in (1, 2, 3) for label in range(10)] + [(4, 0, 12), (4, 8, 12), (5, 4, 12), (6, 1, 12), (7, 0, 64), (7, 9, 64), (23, 2, 28), (35, 5, 28), (13, 0, 28), (29, 3, 28)]


class Cv2StandIn(types.ModuleType):
    BORDER_CONSTANT = 0

    def __init__(self):
        super().__init__("cv2")
        self.calls = []

    def _rec(self, name, params, src, out):
        p = np.zeros(10)
        p[:len(params)] = params
        self.calls.append((name, p, np.array(src), np.array(out)))
        return out

    def getRotationMatrix2D(self, center, angle, scale):
        return ar.rotation_matrix(center, angle, scale)

    def warpAffine(self, img, matrix, dsize, borderValue=0):
        assert dsize == (img.shape[1], img.shape[0])
        return self._rec("warpAffine", list(np.asarray(matrix, np.float64).reshape(-1)) + [borderValue], img, sr.warp_affine_const(img, matrix, borderValue))

    def getPerspectiveTransform(self, src, dst):
        return ar.perspective_matrix(src, dst)

    def warpPerspective(self, img, matrix, dsize, borderValue=0):
        assert dsize == (img.shape[1], img.shape[0])
        return self._rec("warpPerspective", list(np.asarray(matrix, np.float64).reshape(-1)) + [borderValue], img, sr.warp_perspective_const(img, matrix, borderValue))

    def resize(self, img, dsize):
        out = warp_ref.resize(img, dsize)
        self.calls.append(("resize", np.array(list(dsize) + [0] * 8, np.float64), np.array(img), None))
        return out

    def copyMakeBorder(self, img, top, bottom, left, right, borderType, value=0):
        assert borderType == self.BORDER_CONSTANT
        out = np.pad(img, ((top, bottom), (left, right)), constant_values=value)
        self.calls.append(("copyMakeBorder", np.array([top, bottom, left, right, value, 0, 0, 0, 0, 0], np.float64), None, np.array(out)))
        return out

    def GaussianBlur(self, img, ksize, sigma):
        assert ksize[0] == ksize[1] and img.dtype == np.uint8
        return self._rec("GaussianBlur", [ksize[0], sigma], img, sr.gauss_blur(img, ksize[0], sr.gaussian_taps_q8(ksize[0], sigma)))

    def erode(self, img, kernel, iterations=1):
        assert kernel.shape == (2, 2) and (kernel == 1).all() and iterations == 1
        return self._rec("erode", [], img, sr.morph(img, False))

    def dilate(self, img, kernel, iterations=1):
        assert kernel.shape == (2, 2) and (kernel == 1).all() and iterations == 1
        return self._rec("dilate", [], img, sr.morph(img, True))


class RandomRecorder:
    """The reference module's `random`: Python's global generator, every draw recorded."""

    def __init__(self):
        self.draws = []

    def _rec(self, v):
        self.draws.append(float(v) if not isinstance(v, str) else float(len(v)))
        return v

    def uniform(self, a, b):
        return self._rec(_random.uniform(a, b))

    def random(self):
        return self._rec(_random.random())

    def randint(self, a, b):
        return self._rec(_random.randint(a, b))

    def choice(self, seq):
        k = _random.choice(range(len(seq)))                   # the same single draw as choice(seq)
        self.draws.append(float(k))
        return seq[k]

    def seed(self, s):
        _random.seed(s)


class NumpyProxy:
    """The reference module's `np`: numpy, but np.random.normal records its sigma."""

    def __init__(self):
        self.normals = []
        outer = self

        class R:
            def normal(self, loc, scale, size):
                outer.normals.append(float(scale))
                return np.random.normal(loc, scale, size)

            def __getattr__(self, name):
                return getattr(np.random, name)
        self.random = R()

    def __getattr__(self, name):
        return getattr(np, name)


def load_reference(path):
    cv2 = Cv2StandIn()
    sys.modules["cv2"] = cv2
    spec = importlib.util.spec_from_file_location("reference_generate_synthetic_v2", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rec, npp = RandomRecorder(), NumpyProxy()
    mod.random, mod.np = rec, npp
    log = {}
    for name in ("generate_paper_background", "add_grid_artifacts"):
        def wrap(name=name, fn=getattr(mod, name)):
            def wrapped(*args, **kwargs):
                out = fn(*args, **kwargs)
                log.setdefault(name, []).append((np.array(args[0]) if name == "add_grid_artifacts" else None, np.array(out)))
                return out
            return wrapped
        setattr(mod, name, wrap())
    return mod, cv2, rec, npp, log


def main():
    from PIL import ImageFont
    mod, cv2, rec, npp, log = load_reference(sys.argv[1])
    font_path = sys.argv[2]
    fonts = [("golden", None)]
    out, cells = {}, []
    for c, (seed, label, size) in enumerate(JOBS):
        _random.seed(seed)
        np.random.seed(seed)
        del cv2.calls[:], rec.draws[:], npp.normals[:]
        log.clear()
        font_size = 0
        if label == 0:
            base = mod.generate_empty_cell(size=size)
        else:
            rec.choice(fonts)                                  # generate_dataset's font choice and size, then the reload
            font_size = rec.randint(16, 24)
            font = ImageFont.truetype(font_path, font_size)
            mask, off = font.getmask2(str(label), mode="L")
            out[f"c{c}_mask"] = np.array(mask, np.uint8).reshape(mask.size[1], mask.size[0])
            out[f"c{c}_glyph"] = np.array(list(off) + list(font.getbbox(str(label), "L")), np.int64)
            base = mod.generate_digit(label, font, size=size, jitter=2)
        n_bg_normals = len(npp.normals)
        result = mod.apply_augmentation(base, is_empty=(label == 0))
        assert result.shape == (size, size) and result.dtype == np.uint8
        out[f"c{c}_draws"] = np.array(rec.draws, np.float64)
        out[f"c{c}_next"] = np.array(_random.random())
        out[f"c{c}_base"], out[f"c{c}_out"] = np.array(base), np.array(result)
        out[f"c{c}_bg"] = log["generate_paper_background"][0][1]
        if "add_grid_artifacts" in log:
            out[f"c{c}_art_in"], out[f"c{c}_art_out"] = log["add_grid_artifacts"][0]
        out[f"c{c}_normal"] = np.array(npp.normals, np.float64).reshape(-1, 1)
        img_calls = [k for k in cv2.calls if k[2] is not None and k[3] is not None]
        out[f"c{c}_cv_names"] = np.array([k[0] for k in cv2.calls])
        out[f"c{c}_cv_params"] = np.stack([k[1] for k in cv2.calls]) if cv2.calls else np.zeros((0, 10))
        out[f"c{c}_cv_img_names"] = np.array([k[0] for k in img_calls])
        out[f"c{c}_cv_in"] = np.stack([k[2] for k in img_calls]) if img_calls else np.zeros((0, size, size), np.uint8)
        out[f"c{c}_cv_out"] = np.stack([k[3] for k in img_calls]) if img_calls else np.zeros((0, size, size), np.uint8)
        cells.append((seed, label, size, font_size, int(not npp.normals), n_bg_normals))
    out["cells"] = np.array(cells, np.int64)
    np.savez_compressed(os.path.join(HERE, "synth_cells_goldens.npz"), **out)
    print(f"{len(cells)} cells written, {sum(c[4] for c in cells)} without an np.random field")


if __name__ == "__main__":
    main()
