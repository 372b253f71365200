#!/usr/bin/env python3
"""MI355X drop-in for the reference's tools/augment_data.py: the same functions, arguments, file names and statistics.

What the reference does one image and one cv2 call at a time is here a *program*: every augmentation draws its scalar parameters on
the host -- from Python's global `random`, with the reference's calls in the reference's order, so random.seed(s) selects the same
operations with the same parameters -- and emits one step record; K22 (csrc/k22_augment.hip, Context.augment) then runs the
programs of a whole batch in one launch, each image staying in LDS from its first step to its last.

The operations that the reference feeds from np.random (add_noise, elastic_transform) take their fields from Philox on the GPU.  At
the point where the reference consumes np.random they draw one 32-bit salt from it, so np.random.seed still selects the fields and
the `random` stream stays aligned with the reference's; the field bits themselves are not NumPy's.

Images are gray uint8 of 4..64 pixels a side, numpy arrays or CUDA tensors (a tensor gives a tensor), as in cv/preprocess_v2.py.
Building programs needs no GPU; running them does, and there is no CPU fallback.

Usage:
    python ml/augment_data.py data/labeled/train --output data/augmented/train
    python ml/augment_data.py data/labeled/train --multiplier 10
"""
import argparse
import ctypes as C
import os
import random
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bootstrap import package  # noqa: E402
sys.path.pop(0)
_pkg = package()
_rt, _nv = _pkg.runtime, _pkg._native

MIN_SIDE, MAX_SIDE = 4, _nv.AUG_MAX_SIDE


def _check_side(h, w):
    if not (MIN_SIDE <= h <= MAX_SIDE and MIN_SIDE <= w <= MAX_SIDE):
        raise ValueError(f"image of {h} x {w}: the augmentation kernel takes sides of {MIN_SIDE}..{MAX_SIDE} pixels")


def _step(op, i=(), d=(), f=()):
    s = np.zeros((), _nv.AUG_STEP_DTYPE)
    s["op"] = op
    s["i"][:len(i)] = i
    if len(f):
        s["f"][:len(f)] = f
    else:
        s["d"][:len(d)] = d
    return s


def _salt():
    """The one draw a field operation makes from np.random, where the reference draws its arrays."""
    return int(np.random.randint(0, 2 ** 32, dtype=np.uint64))


def _as_i32(v):
    return v - (1 << 32) if v >= (1 << 31) else v


# ---- the draws: the reference's calls to `random`, in its order, -> one step record (None: the image is returned as it is) ----
def _draw_rotate(h, w, angle_range=(-15, 15)):
    angle = random.uniform(*angle_range)
    m = (C.c_double * 6)()
    _nv.check(_nv.lib().sv_augment_rotation_matrix(float(w // 2), float(h // 2), angle, 1.0, m), "sv_augment_rotation_matrix")
    return _step(_nv.AUG_AFFINE, d=list(m))


def _draw_perspective_warp(h, w, distortion=0.1):
    src = np.float32([[0, 0], [w, 0], [w, h], [0, h]])
    dst = src.copy()
    for i in range(4):
        dst[i][0] += random.uniform(-distortion, distortion) * w      # float32 +=, as the reference's array does it
        dst[i][1] += random.uniform(-distortion, distortion) * h
    m = (C.c_double * 9)()
    _nv.check(_nv.lib().sv_augment_perspective_matrix(src.ctypes.data, dst.ctypes.data, m), "sv_augment_perspective_matrix")
    return _step(_nv.AUG_PERSPECTIVE, d=list(m))


def _draw_adjust_brightness(h, w, range_pct=(-0.2, 0.2)):
    return _step(_nv.AUG_BRIGHTNESS, d=[random.uniform(*range_pct) * 255])


def _draw_adjust_contrast(h, w, range_factor=(0.8, 1.2)):
    return _step(_nv.AUG_CONTRAST, d=[random.uniform(*range_factor)])


def _draw_gaussian_blur(h, w, kernel_range=(1, 3)):
    k = random.choice(range(kernel_range[0], kernel_range[1] + 1, 2))
    if k < 1:
        k = 1
    if k % 2 == 0:
        k += 1
    return _step(_nv.AUG_BLUR, i=[k])


def _draw_add_noise(h, w, noise_type="gaussian", intensity=0.05):
    if noise_type == "gaussian":
        return _step(_nv.AUG_NOISE_GAUSS, i=[0, 0, 0, 0, _as_i32(_salt())], d=[intensity * 255])
    if noise_type == "salt_pepper":
        return _step(_nv.AUG_NOISE_SP, i=[0, 0, 0, 0, _as_i32(_salt())], d=[intensity / 2])
    return None


def _draw_elastic_transform(h, w, alpha=10, sigma=3):
    taps = (C.c_float * (_nv.AUG_MAX_RADIUS + 1))()
    radius = C.c_int()
    _nv.check(_nv.lib().sv_augment_elastic_taps(float(sigma), taps, len(taps), C.byref(radius)), "sv_augment_elastic_taps")
    r = radius.value
    return _step(_nv.AUG_ELASTIC, i=[r, 0, 0, 0, _as_i32(_salt())], f=[np.float32(alpha)] + list(taps)[:r + 1])


def _draw_random_erasing(h, w, probability=0.5, area_range=(0.02, 0.1)):
    if random.random() > probability:
        return None
    area = h * w
    target_area = random.uniform(*area_range) * area
    aspect_ratio = random.uniform(0.3, 3.0)
    eh = int(round(np.sqrt(target_area * aspect_ratio)))
    ew = int(round(np.sqrt(target_area / aspect_ratio)))
    if eh >= h or ew >= w:
        return None
    x = random.randint(0, w - ew)
    y = random.randint(0, h - eh)
    return _step(_nv.AUG_FILL_RECT, i=[x, y, ew, eh, random.randint(0, 255)])


def _draw_translate(h, w, max_shift=0.1):
    dx = int(random.uniform(-max_shift, max_shift) * w)
    dy = int(random.uniform(-max_shift, max_shift) * h)
    return _step(_nv.AUG_AFFINE, d=[1, 0, dx, 0, 1, dy])


def _draw_scale(h, w, scale_range=(0.9, 1.1)):
    factor = random.uniform(*scale_range)
    new_h, new_w = int(h * factor), int(w * factor)
    return _step(_nv.AUG_SCALE, i=[new_w, new_h, 1 if factor > 1 else 0])


# ---- running programs -------------------------------------------------------------------------------------------------------
def _pack(chains):
    steps = np.zeros((len(chains), _nv.AUG_MAX_STEPS), _nv.AUG_STEP_DTYPE)
    for k, chain in enumerate(chains):
        if len(chain) > _nv.AUG_MAX_STEPS:
            raise ValueError(f"{len(chain)} augmentations in one chain; the kernel runs at most {_nv.AUG_MAX_STEPS}")
        for j, s in enumerate(chain):
            steps[k, j] = s
    return steps, np.array([len(c) for c in chains], np.int32)


def _gray(image):
    shape = tuple(image.shape)
    if len(shape) != 2:
        raise ValueError(f"expected a gray image [H,W], got shape {list(shape)}")
    _check_side(*shape)
    return shape


def _run_one(image, chain, seed=0, index=0):
    """One image through one chain of step records (None entries left out)."""
    chain = [s for s in chain if s is not None]
    if not chain:
        return image
    ctx = _rt.default_context(image.device if isinstance(image, torch.Tensor) else None)
    d, was_tensor = _rt._to_dev(image, ctx)
    steps, n_steps = _pack([chain])
    out = ctx.augment(d[None], steps, n_steps, np.zeros(1, np.int32), seed=seed or 0, index_base=index)
    return _rt._back(out[0], was_tensor)


class Augmentation:
    """One entry of an augmentation pipeline.  Called with an image it draws its parameters and applies itself, as the reference's
    lambdas do; .draw(h, w) makes the same draws and returns the step record without running anything (None when this draw leaves
    the image as it is), which is what lets augment_image and augment_batch run a whole chain, or a whole batch, in one launch."""

    def __init__(self, name, draw, *args):
        self.name, self._draw, self._args = name, draw, args

    def draw(self, h, w):
        return self._draw(h, w, *self._args)

    def __call__(self, image):
        h, w = _gray(image)
        return _run_one(image, [self.draw(h, w)])

    def __repr__(self):
        return f"Augmentation({self.name}{self._args})"


def _function(name, draw):
    def fn(image, *args, **kwargs):
        h, w = _gray(image)
        return _run_one(image, [draw(h, w, *args, **kwargs)])
    fn.__name__ = fn.__qualname__ = name
    fn.__doc__ = f"{name} of the reference, one launch of K22 for one image."
    return fn


rotate = _function("rotate", _draw_rotate)
perspective_warp = _function("perspective_warp", _draw_perspective_warp)
adjust_brightness = _function("adjust_brightness", _draw_adjust_brightness)
adjust_contrast = _function("adjust_contrast", _draw_adjust_contrast)
gaussian_blur = _function("gaussian_blur", _draw_gaussian_blur)
add_noise = _function("add_noise", _draw_add_noise)
elastic_transform = _function("elastic_transform", _draw_elastic_transform)
random_erasing = _function("random_erasing", _draw_random_erasing)
translate = _function("translate", _draw_translate)
scale = _function("scale", _draw_scale)


def create_augmentation_pipeline(intensity="medium"):
    """Create augmentation pipeline based on intensity level: a list of Augmentation objects."""
    A = Augmentation
    if intensity == "light":
        return [A("rotate", _draw_rotate, (-5, 5)), A("adjust_brightness", _draw_adjust_brightness, (-0.1, 0.1)),
                A("adjust_contrast", _draw_adjust_contrast, (0.9, 1.1))]
    if intensity == "medium":
        return [A("rotate", _draw_rotate, (-10, 10)), A("perspective_warp", _draw_perspective_warp, 0.05),
                A("adjust_brightness", _draw_adjust_brightness, (-0.15, 0.15)), A("adjust_contrast", _draw_adjust_contrast, (0.85, 1.15)),
                A("gaussian_blur", _draw_gaussian_blur, (1, 3)), A("translate", _draw_translate, 0.05)]
    if intensity == "heavy":
        return [A("rotate", _draw_rotate, (-15, 15)), A("perspective_warp", _draw_perspective_warp, 0.1),
                A("adjust_brightness", _draw_adjust_brightness, (-0.2, 0.2)), A("adjust_contrast", _draw_adjust_contrast, (0.8, 1.2)),
                A("gaussian_blur", _draw_gaussian_blur, (1, 5)), A("add_noise", _draw_add_noise, "gaussian", 0.03),
                A("elastic_transform", _draw_elastic_transform, 8, 3), A("translate", _draw_translate, 0.1),
                A("scale", _draw_scale, (0.9, 1.1)), A("random_erasing", _draw_random_erasing, 0.3)]
    raise ValueError(f"Unknown intensity: {intensity}")


def draw_chain(h, w, augmentations, n_augmentations=3):
    """augment_image's draws for one h x w image: the sample of the pipeline, then every selected entry's own draws in order.
    -> the list of step records (identity draws left out).  Every entry must have .draw."""
    selected = random.sample(augmentations, min(n_augmentations, len(augmentations)))
    return [s for s in (aug.draw(h, w) for aug in selected) if s is not None]


def build_program(n_images, h, w, multiplier, augmentations, n_augmentations=3):
    """The program of process_directory's loop over n_images images of h x w: image by image, `multiplier` chains each.
    -> (steps, n_steps, src_index) as Context.augment takes them.  Needs no GPU."""
    _check_side(h, w)
    chains = [draw_chain(h, w, augmentations, n_augmentations) for _ in range(n_images) for _ in range(multiplier)]
    steps, n_steps = _pack(chains)
    return steps, n_steps, np.repeat(np.arange(n_images, dtype=np.int32), multiplier)


def augment_image(image, augmentations, n_augmentations=3, *, seed=0, index=0):
    """Apply random subset of augmentations to image.  When every entry can emit its step record (.draw) the chain is one launch;
    foreign callables are called one by one, as the reference does.  seed and index (beyond the reference's signature) key the
    random fields: the image that augment_batch puts at output `index` under `seed`."""
    if all(hasattr(a, "draw") for a in augmentations):
        h, w = _gray(image)
        chain = draw_chain(h, w, augmentations, n_augmentations)
        if not chain:
            return image.clone() if isinstance(image, torch.Tensor) else image.copy()
        return _run_one(image, chain, seed, index)
    result = image.clone() if isinstance(image, torch.Tensor) else image.copy()
    for aug in random.sample(augmentations, min(n_augmentations, len(augmentations))):
        result = aug(result)
    return result


def augment_batch(images, multiplier=1, intensity="medium", n_augmentations=3, seed=None):
    """images u8 [N,H,W] (CUDA tensor or array) -> (out [N*multiplier,H,W], src_index): `multiplier` augmented copies of every image,
    one program build on the host and one launch.  Byte-identical to augment_image(images[n], pipeline, n_augmentations, seed=seed,
    index=n*multiplier + i) called in that order under the same random and np.random seeds."""
    ctx = _rt.default_context(images.device if isinstance(images, torch.Tensor) else None)
    d, was_tensor = _rt._to_dev(images, ctx)
    if d.dim() != 3:
        raise ValueError(f"expected images [N,H,W], got shape {list(d.shape)}")
    n, h, w = d.shape
    steps, n_steps, src_index = build_program(n, h, w, multiplier, create_augmentation_pipeline(intensity), n_augmentations)
    out = ctx.augment(d, steps, n_steps, src_index, seed=seed or 0)
    return _rt._back(out, was_tensor), src_index


def _read_gray(path, ctx):
    from sudoku_vision_amd import imgcodecs as ic
    if str(path).lower().endswith(".png"):
        img = ic.imread_png(str(path), device=True, ctx=ctx)
        if img is not None and img.dim() == 3:                # PNGs decode to BGR; a gray file has three equal channels
            img = ctx.gray(img[None])[0] if img.shape[2] == 3 else img[:, :, 0]
        return img
    return ic.imread(str(path), device=True, ctx=ctx, gray=True)


def _write(path, img, ctx):
    from sudoku_vision_amd import imgcodecs as ic
    if str(path).lower().endswith(".png"):
        return ic.imwrite_png(str(path), img, ctx=ctx)
    return ic.imwrite(str(path), img, ctx=ctx)


def process_directory(input_dir, output_dir, multiplier=10, intensity="medium", preserve_originals=True):
    """Process all images in a class directory structure; the reference's file names and statistics dictionary.  The draws are made
    image by image in file order; the images of a class are then grouped by size and every group is augmented in one launch."""
    input_dir, output_dir = Path(input_dir), Path(output_dir)
    augmentations = create_augmentation_pipeline(intensity)
    ctx = _rt.default_context()
    stats = {"originals": 0, "augmented": 0, "by_class": {}}
    class_dirs = [d for d in input_dir.iterdir() if d.is_dir() and d.name.isdigit()]
    for class_dir in sorted(class_dirs, key=lambda d: int(d.name)):
        class_label = class_dir.name
        out_class_dir = output_dir / class_label
        out_class_dir.mkdir(parents=True, exist_ok=True)
        class_stats = {"originals": 0, "augmented": 0}
        image_files = list(class_dir.glob("*.png")) + list(class_dir.glob("*.jpg"))
        groups = {}                                           # (h, w) -> [images, chains, names]
        for img_path in image_files:
            img = _read_gray(img_path, ctx)
            if img is None:
                continue
            h, w = img.shape
            _check_side(h, w)
            class_stats["originals"] += 1
            if preserve_originals:
                _write(out_class_dir / f"orig_{img_path.name}", img, ctx)
            g = groups.setdefault((h, w), [[], [], []])
            g[0].append(img)
            for i in range(multiplier):
                g[1].append((len(g[0]) - 1, draw_chain(h, w, augmentations)))
                g[2].append(out_class_dir / f"aug_{i}_{img_path.name}")
                class_stats["augmented"] += 1
        for images, chains, names in groups.values():
            if not chains:
                continue
            steps, n_steps = _pack([c for _, c in chains])
            out = ctx.augment(torch.stack(images), steps, n_steps, np.array([k for k, _ in chains], np.int32))
            for name, img in zip(names, out):
                _write(name, img, ctx)
        stats["by_class"][class_label] = class_stats
        stats["originals"] += class_stats["originals"]
        stats["augmented"] += class_stats["augmented"]
        print(f"  Class {class_label}: {class_stats['originals']} -> {class_stats['augmented']} augmented")
    return stats


def preview_augmentations(image_path, output_path, intensity="medium"):
    """Generate preview grid showing augmentation effects: the original and 15 augmented copies, 56 x 56 each."""
    ctx = _rt.default_context()
    img = _read_gray(image_path, ctx)
    if img is None:
        print(f"Error: Could not load {image_path}")
        return
    augmentations = create_augmentation_pipeline(intensity)
    grid_size, cell_size = 4, 56
    grid = torch.zeros((cell_size * grid_size, cell_size * grid_size), dtype=torch.uint8, device=ctx.device)
    grid[0:cell_size, 0:cell_size] = ctx.resize_linear(img, (cell_size, cell_size))
    for i in range(1, grid_size * grid_size):
        row, col = divmod(i, grid_size)
        augmented = augment_image(img, augmentations)
        grid[row * cell_size:(row + 1) * cell_size, col * cell_size:(col + 1) * cell_size] = ctx.resize_linear(augmented, (cell_size, cell_size))
    _write(output_path, grid, ctx)
    print(f"Preview saved to: {output_path}")


def main():
    parser = argparse.ArgumentParser(description="Augment training data for improved model robustness")
    parser.add_argument("input_dir", type=Path, help="Input directory with class subdirectories")
    parser.add_argument("--output", "-o", type=Path, default=None, help="Output directory (default: input_dir_augmented)")
    parser.add_argument("--multiplier", "-m", type=int, default=10, help="Number of augmented copies per original (default: 10)")
    parser.add_argument("--intensity", "-i", choices=["light", "medium", "heavy"], default="medium", help="Augmentation intensity (default: medium)")
    parser.add_argument("--no-originals", action="store_true", help="Don't include original images in output")
    parser.add_argument("--preview", type=Path, help="Generate preview for a single image instead of processing")
    parser.add_argument("--seed", type=int, default=None, help="Random seed for reproducibility")
    args = parser.parse_args()

    if args.seed is not None:
        random.seed(args.seed)
        np.random.seed(args.seed)
    if not args.input_dir.exists():
        print(f"Error: Input directory does not exist: {args.input_dir}")
        sys.exit(1)
    if args.preview:
        preview_augmentations(args.preview, args.output or Path("augmentation_preview.png"), args.intensity)
        return
    output_dir = args.output or Path(str(args.input_dir) + "_augmented")
    print("Data Augmentation Pipeline")
    print("=" * 50)
    print(f"Input: {args.input_dir}")
    print(f"Output: {output_dir}")
    print(f"Multiplier: {args.multiplier}x")
    print(f"Intensity: {args.intensity}")
    print(f"Include originals: {not args.no_originals}")
    print("=" * 50)
    print("\nProcessing...")
    stats = process_directory(args.input_dir, output_dir, multiplier=args.multiplier, intensity=args.intensity, preserve_originals=not args.no_originals)
    print("\n" + "=" * 50)
    print("AUGMENTATION COMPLETE")
    print("=" * 50)
    print(f"Original images: {stats['originals']}")
    print(f"Augmented images: {stats['augmented']}")
    print(f"Total output: {stats['originals'] + stats['augmented'] if not args.no_originals else stats['augmented']}")
    print(f"Output directory: {output_dir}")


if __name__ == "__main__":
    main()
