#!/usr/bin/env python3
"""MI355X drop-in for the reference's ml/generate_synthetic_v2.py: the same functions, arguments, directory tree and metadata.

What the reference does one image and one cv2 call at a time is here a *job*: every function makes the reference's draws from Python's
global `random`, in the reference's order, and writes them into a cell record (background, grain, artefacts, smudge, glyph) and a step
program (the eight augmentations); K23 (csrc/k23_synth_cells.hip, Context.synth_cells) then draws every cell of the job in one launch.
Where the reference consumes np.random (the Gaussian fields of the textured and noisy papers and of the noise step) one 32-bit salt is
drawn from np.random instead and the field is the kernel's Philox field: random.seed(s) selects the same backgrounds, fonts, sizes,
jitters, inks and augmentation parameters as in the reference, while the field bits are Philox's, not NumPy's.

Glyphs are rasterised on the host by Pillow / FreeType, once per (font, size, digit): the kernel reads their coverage masks from an
atlas.  Pillow is needed for nothing else; build_cells takes any object with a .glyph(digit) method in place of a font.

Beyond the reference: build_cells (the job of a list of labels, no GPU needed) and generate_batch (labels -> u8 [N, size, size] on the
device in one launch, byte-identical to the loop of the single calls under the same seeds).

Usage:
    python ml/generate_synthetic_v2.py --output data/synthetic_v2 --num-per-class 10000
    python ml/generate_synthetic_v2.py --preview
"""
import argparse
import ctypes as C
import json
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

try:
    from PIL import ImageFont
except ImportError:                                           # a caller may still pass its own glyph sources
    ImageFont = None

MIN_SIDE, MAX_SIDE = 4, _nv.AUG_MAX_SIDE
PADDING = 10                                                  # the reference's canvas padding around the cell

# =============================================================================
# Font Discovery
# =============================================================================

PREFERRED_FONTS = [
    "Arial", "Arial Black", "Arial Narrow",
    "Helvetica", "Helvetica Neue", "Helvetica Neue Medium",
    "Verdana", "Tahoma", "Trebuchet MS",
    "Futura", "Gill Sans", "Optima",
    "Times New Roman", "Georgia", "Palatino",
    "Garamond", "Baskerville", "Didot",
    "Courier New", "Courier", "Menlo", "Monaco",
    "SF Mono", "Consolas", "Lucida Console",
    "SF Pro Display", "SF Pro Text",
    ".SF NS Display", ".SF NS Text",
]

FONT_SEARCH_PATHS = [
    "/System/Library/Fonts/",
    "/Library/Fonts/",
    "~/Library/Fonts/",
    "/System/Library/Fonts/Supplemental/",
]
_extra_dirs = []                                              # find_available_fonts(extra_dirs=...) adds to the search paths


def _search_paths():
    return FONT_SEARCH_PATHS + [d for d in _extra_dirs if d not in FONT_SEARCH_PATHS]


def find_available_fonts(size=24, extra_dirs=()):
    """Find all available fonts on the system: [(name, font)].  extra_dirs: more directories to search, after the reference's."""
    for d in extra_dirs:
        if str(d) not in _extra_dirs:
            _extra_dirs.append(str(d))
    found_fonts = []
    for font_name in PREFERRED_FONTS:
        font = _try_load_font(font_name, size)
        if font:
            found_fonts.append((font_name, font))
    for path in _search_paths():
        font_dir = Path(path).expanduser()
        if font_dir.exists():
            for pattern in ("*.ttf", "*.ttc"):
                for font_file in font_dir.glob(pattern):
                    try:
                        found_fonts.append((font_file.stem, ImageFont.truetype(str(font_file), size)))
                    except Exception:
                        pass
    seen, unique_fonts = set(), []
    for name, font in found_fonts:
        if name not in seen:
            seen.add(name)
            unique_fonts.append((name, font))
    return unique_fonts


def _try_load_font(font_name, size):
    """Try to load a font by name."""
    if ImageFont is None:
        return None
    for name in [font_name] + [font_name + ext for ext in (".ttf", ".ttc", ".otf")]:
        try:
            return ImageFont.truetype(name, size)
        except Exception:
            pass
    for path in _search_paths():
        font_dir = Path(path).expanduser()
        for ext in (".ttf", ".ttc", ".otf"):
            font_path = font_dir / (font_name + ext)
            if font_path.exists():
                try:
                    return ImageFont.truetype(str(font_path), size)
                except Exception:
                    pass
    return None


def _default_fonts():
    print("Warning: No fonts found, using default")
    return [("default", ImageFont.load_default())]


# ---- glyphs: what Pillow draws for str(digit), cached per (font, size, digit) ----------------------------------------------------
_glyph_cache = {}


def _glyph(font, digit):
    """-> (mask u8 [h, w], (off_x, off_y), bbox): the coverage mask ImageDraw.text pastes at (x + off_x, y + off_y), and textbbox((0, 0))."""
    if hasattr(font, "glyph"):
        return font.glyph(digit)
    path = getattr(font, "path", None)
    key = (path if isinstance(path, str) else id(font), getattr(font, "size", None), getattr(font, "index", 0), int(digit))
    hit = _glyph_cache.get(key)
    if hit is None:
        text = str(digit)
        if hasattr(font, "getmask2"):
            mask, off = font.getmask2(text, mode="L")
        else:
            mask, off = font.getmask(text, "L"), (0, 0)
        w, h = mask.size
        arr = np.array(mask, np.uint8).reshape(h, w) if w and h else np.zeros((1, 1), np.uint8)
        hit = _glyph_cache[key] = (arr, (int(off[0]), int(off[1])), tuple(int(v) for v in font.getbbox(text, "L")))
    return hit


class Job:
    """The cells of one launch while they are drawn: records, programs and the atlas of the glyphs they use."""

    def __init__(self, size):
        if not MIN_SIDE <= size <= MAX_SIDE:
            raise ValueError(f"cells of {size} x {size}: the generator kernel takes sides of {MIN_SIDE}..{MAX_SIDE} pixels")
        self.size, self.cells, self.chains, self.masks, self._slots = size, [], [], [], {}

    def slot(self, mask):
        key = (mask.shape, mask.tobytes())
        if key not in self._slots:
            G = _nv.SYN_GLYPH_SIDE
            if mask.shape[0] > G or mask.shape[1] > G:
                raise ValueError(f"glyph mask of {mask.shape[1]} x {mask.shape[0]} pixels: the atlas takes at most {G} x {G} (font sizes up to 24)")
            self._slots[key] = len(self.masks)
            self.masks.append(mask)
        return self._slots[key]

    def arrays(self):
        cells = np.zeros(len(self.cells), _nv.SYN_CELL_DTYPE)
        for k, c in enumerate(self.cells):
            cells[k] = c
        steps = np.zeros((len(self.chains), _nv.AUG_MAX_STEPS), _nv.AUG_STEP_DTYPE)
        for k, chain in enumerate(self.chains):
            for j, s in enumerate(chain):
                steps[k, j] = s
        return cells, steps, np.array([len(c) for c in self.chains], np.int32), _rt.Context.synth_atlas(self.masks)


def _step(op, i=(), d=()):
    s = np.zeros((), _nv.AUG_STEP_DTYPE)
    s["op"] = op
    s["i"][:len(i)] = i
    s["d"][:len(d)] = d
    return s


def _salt():
    """The one draw a field makes from np.random, where the reference draws its array."""
    v = int(np.random.randint(0, 2 ** 32, dtype=np.uint64))
    return v - (1 << 32) if v >= (1 << 31) else v


def _new_cell():
    c = np.zeros((), _nv.SYN_CELL_DTYPE)
    c["glyph_slot"] = -1
    return c


# ---- the draws: the reference's calls to `random`, in its order, into a cell record -----------------------------------------------
def _draw_background(c, size):
    variation = random.choice(["plain", "textured", "gradient", "noisy"])
    if variation == "plain":
        c["bg_kind"], c["bg_value"] = _nv.SYN_BG_PLAIN, random.randint(235, 255)
    elif variation == "textured":
        c["bg_kind"], c["bg_value"] = _nv.SYN_BG_TEXTURED, random.randint(240, 250)
        c["bg_d"][0] = random.uniform(2, 5)                   # drawn before np.random is touched: the argument order of the reference's call
        c["bg_salt"] = _salt()
        if random.random() > 0.5:
            stride = random.randint(2, 4)
            bits = 0
            for k, _ in enumerate(range(0, size, stride)):
                bits |= random.randint(1, 3) << (2 * k)
            c["grain_stride"], c["grain_d"] = stride, (bits & 0xffffffff, bits >> 32)
    elif variation == "gradient":
        c["bg_kind"], c["bg_value"] = _nv.SYN_BG_GRADIENT, random.randint(240, 250)
        direction = random.choice(["h", "v", "radial"])
        strength = random.uniform(3, 10)
        if direction == "radial":
            c["grad_dir"], c["bg_d"][0] = 2, strength
        else:
            _, step = np.linspace(-strength, strength, size, retstep=True)       # numpy's own terms
            c["grad_dir"], c["bg_d"] = (0 if direction == "h" else 1), (-strength, step, strength)
    else:
        c["bg_kind"], c["bg_value"] = _nv.SYN_BG_NOISY, random.randint(245, 255)
        c["bg_d"][0] = random.uniform(3, 8)
        c["bg_salt"] = _salt()


def _draw_grid_artifacts(c):
    c["art_dark"] = random.randint(180, 220)
    c["art_width"] = random.randint(1, 2)
    c["art_edges"] = sum(bit for bit in (1, 2, 4, 8) if random.random() > 0.6)


def _draw_digit(job, digit, font, jitter=2):
    c = _new_cell()
    size = job.size
    _draw_background(c, size)
    mask, off, bbox = _glyph(font, digit)
    img_size = size + PADDING * 2
    x = (img_size - (bbox[2] - bbox[0])) // 2 + random.randint(-jitter, jitter)
    y = (img_size - (bbox[3] - bbox[1])) // 2 + random.randint(-jitter, jitter) - bbox[1]
    c["glyph_ink"] = random.randint(0, 30)
    c["glyph_slot"], c["glyph_x"], c["glyph_y"] = job.slot(mask), x + off[0] - PADDING, y + off[1] - PADDING
    return c


def _draw_empty_cell(job):
    c = _new_cell()
    size = job.size
    _draw_background(c, size)
    if random.random() > 0.5:
        _draw_grid_artifacts(c)
    if random.random() > 0.8:
        side = random.randint(2, 5)
        x = random.randint(0, size - side)
        y = random.randint(0, size - side)
        c["smudge"] = (x, y, side, random.randint(210, 240))
    return c


def _draw_augmentation(h, w, is_empty=False):
    """apply_augmentation's draws -> its step records, in order."""
    lib, chain = _nv.lib(), []
    if random.random() > 0.3:
        angle = random.uniform(-8, 8) if is_empty else random.uniform(-10, 10)
        m = (C.c_double * 6)()
        _nv.check(lib.sv_augment_rotation_matrix(float(w // 2), float(h // 2), angle, 1.0, m), "sv_augment_rotation_matrix")
        chain.append(_step(_nv.SYN_AFFINE_CONST, i=[255], d=list(m)))
    if random.random() > 0.4:
        scale = random.uniform(0.9, 1.1)
        new_size = max(1, int(w * scale))
        chain.append(_step(_nv.SYN_SCALE_PAD, i=[new_size, new_size, 1 if new_size > w else 0, 255]))
    if random.random() > 0.5:
        ksize = random.choice([3, 5])
        sigma = random.uniform(0.3, 1.0)
        taps = (C.c_int32 * 3)()
        _nv.check(lib.sv_synth_gaussian_taps_q8(ksize, sigma, taps), "sv_synth_gaussian_taps_q8")
        chain.append(_step(_nv.SYN_GAUSS_BLUR, i=[ksize] + list(taps)))
    if random.random() > 0.4:
        chain.append(_step(_nv.AUG_BRIGHTNESS, d=[random.uniform(-15, 15)]))
    if random.random() > 0.4:
        chain.append(_step(_nv.AUG_CONTRAST, d=[random.uniform(0.85, 1.15)]))
    if random.random() > 0.5:
        noise_sigma = random.uniform(2, 8)
        chain.append(_step(_nv.AUG_NOISE_GAUSS, i=[0, 0, 0, 0, _salt()], d=[noise_sigma]))
    if random.random() > 0.7:
        strength = random.uniform(1, 2.5)
        pts1 = np.float32([[0, 0], [w, 0], [w, h], [0, h]])
        pts2 = np.float32([
            [random.uniform(0, strength), random.uniform(0, strength)],
            [w - random.uniform(0, strength), random.uniform(0, strength)],
            [w - random.uniform(0, strength), h - random.uniform(0, strength)],
            [random.uniform(0, strength), h - random.uniform(0, strength)]
        ])
        m = (C.c_double * 9)()
        _nv.check(lib.sv_augment_perspective_matrix(pts1.ctypes.data, pts2.ctypes.data, m), "sv_augment_perspective_matrix")
        chain.append(_step(_nv.SYN_PERSPECTIVE_CONST, i=[255], d=list(m)))
    if not is_empty and random.random() > 0.8:
        chain.append(_step(_nv.SYN_ERODE if random.random() > 0.5 else _nv.SYN_DILATE))
    return chain


def pick_font(fonts):
    """generate_dataset's choice of a font for one digit cell: a font of the list, reloaded at a random size of 16..24."""
    font_name, font = random.choice(fonts)
    font_size = random.randint(16, 24)
    return _try_load_font(font_name, font_size) or font


# ---- running jobs -------------------------------------------------------------------------------------------------------------
def _launch(job, seed=0, index=0, prev=None, device=False):
    ctx = _rt.default_context(prev.device if isinstance(prev, torch.Tensor) else None)
    cells, steps, n_steps, atlas = job.arrays()
    out = None
    if prev is not None:
        out = _rt._to_dev(prev, ctx)[0].to(torch.uint8).reshape(len(cells), job.size, job.size).contiguous().clone()
    res = ctx.synth_cells(cells, steps, n_steps, job.size, atlas, seed=seed or 0, index_base=index, out=out)
    return res if device else res.cpu().numpy()


def _keep_job(img):
    shape = tuple(img.shape)
    if len(shape) != 2 or shape[0] != shape[1]:
        raise ValueError(f"expected a square gray cell [S,S], got shape {list(shape)}")
    job = Job(shape[0])
    c = _new_cell()
    c["bg_kind"] = _nv.SYN_BG_KEEP
    job.cells.append(c)
    job.chains.append([])
    return job


def generate_paper_background(size=28, *, seed=0, index=0):
    """Generate realistic paper texture background.  One launch."""
    job = Job(size)
    c = _new_cell()
    _draw_background(c, size)
    job.cells.append(c)
    job.chains.append([])
    return _launch(job, seed, index)[0]


def add_grid_artifacts(img, *, seed=0, index=0):
    """Add grid line artifacts at cell edges.  One launch: the image enters as the kernel's kept background."""
    job = _keep_job(img)
    _draw_grid_artifacts(job.cells[0])
    out = _launch(job, seed, index, prev=img, device=isinstance(img, torch.Tensor))
    return out[0]


def generate_digit(digit, font, size=28, jitter=2, *, seed=0, index=0):
    """Generate a single digit image with paper background.  One launch."""
    job = Job(size)
    job.cells.append(_draw_digit(job, digit, font, jitter))
    job.chains.append([])
    return _launch(job, seed, index)[0]


def generate_empty_cell(size=28, *, seed=0, index=0):
    """Generate an empty cell with possible artifacts.  One launch."""
    job = Job(size)
    job.cells.append(_draw_empty_cell(job))
    job.chains.append([])
    return _launch(job, seed, index)[0]


def apply_augmentation(img, is_empty=False, *, seed=0, index=0):
    """Apply random augmentations to simulate real-world conditions.  One launch for the whole chain."""
    job = _keep_job(img)
    job.chains[0] = _draw_augmentation(job.size, job.size, is_empty)
    out = _launch(job, seed, index, prev=img, device=isinstance(img, torch.Tensor))
    return out[0]


def _draw_labels(job, labels, fonts):
    for label in labels:
        if int(label) == 0:
            job.cells.append(_draw_empty_cell(job))
            job.chains.append(_draw_augmentation(job.size, job.size, is_empty=True))
        else:
            job.cells.append(_draw_digit(job, int(label), pick_font(fonts), 2))
            job.chains.append(_draw_augmentation(job.size, job.size, is_empty=False))


def build_cells(labels, fonts, size=28):
    """The job of one cell per label (0: an empty cell; 1..9: that digit), drawn label by label in generate_dataset's order: the font
    choice, the cell's draws, then its augmentation's.  -> (cells, steps, n_steps, atlas) as Context.synth_cells takes them.  Needs no GPU."""
    job = Job(size)
    _draw_labels(job, labels, fonts)
    return job.arrays()


def generate_batch(labels, fonts=None, size=28, seed=None, index_base=0):
    """labels -> u8 [N, size, size] on the device in one launch.  Byte-identical to the loop, label by label, of generate_empty_cell or
    generate_digit(label, pick_font(fonts)) followed by apply_augmentation, each with seed=seed and index=index_base + n."""
    if fonts is None:
        fonts = find_available_fonts(size=22) or _default_fonts()
    ctx = _rt.default_context()
    cells, steps, n_steps, atlas = build_cells(labels, fonts, size)
    return ctx.synth_cells(cells, steps, n_steps, size, atlas, seed=seed or 0, index_base=index_base)


# =============================================================================
# Dataset Generation
# =============================================================================

def generate_dataset(output_dir, num_per_class=10000, val_ratio=0.1, size=28, seed=42, fonts=None):
    """Generate the full synthetic dataset: the reference's tree, file names and metadata.json.  The draws are made class by class and
    image by image in the reference's order; every class is one launch.  fonts: a list to use instead of the discovered ones."""
    from sudoku_vision_amd import imgcodecs as ic
    output_dir = Path(output_dir)
    random.seed(seed)
    np.random.seed(seed)
    ctx = _rt.default_context()
    train_dir, val_dir = output_dir / "train", output_dir / "val"
    for split_dir in [train_dir, val_dir]:
        for digit in range(10):
            (split_dir / str(digit)).mkdir(parents=True, exist_ok=True)
    discovery_size = random.randint(18, 24)
    if fonts is None:
        fonts = find_available_fonts(size=discovery_size)
    print(f"Found {len(fonts)} fonts")
    if not fonts:
        fonts = _default_fonts()
    stats = {
        "total_generated": 0,
        "train_count": 0,
        "val_count": 0,
        "per_class": {str(d): {"train": 0, "val": 0} for d in range(10)},
        "fonts_used": [f[0] for f in fonts[:20]],
    }
    num_val = int(num_per_class * val_ratio)
    num_train = num_per_class - num_val
    for digit in range(10):
        print(f"Generating class {digit}...", end=" ", flush=True)
        if num_per_class > 0:
            cells, steps, n_steps, atlas = build_cells([digit] * num_per_class, fonts, size)
            out = ctx.synth_cells(cells, steps, n_steps, size, atlas, seed=seed, index_base=digit * num_per_class)
            for i in range(num_per_class):
                is_val = i < num_val
                split_dir, split_name = (val_dir, "val") if is_val else (train_dir, "train")
                ic.imwrite_png(str(split_dir / str(digit) / f"{digit}_{i:06d}.png"), out[i], ctx=ctx)
                stats["total_generated"] += 1
                stats[f"{split_name}_count"] += 1
                stats["per_class"][str(digit)][split_name] += 1
        print(f"done ({num_train} train, {num_val} val)")
    metadata = {"size": size, "num_per_class": num_per_class, "val_ratio": val_ratio, "seed": seed, "stats": stats}
    with open(output_dir / "metadata.json", "w") as f:
        json.dump(metadata, f, indent=2)
    return metadata


def generate_preview(output_path, size=28, fonts=None):
    """Generate a preview grid showing sample images from each class: 10 x 5 cells at twice their size, one launch for all fifty."""
    from sudoku_vision_amd import imgcodecs as ic
    if fonts is None:
        fonts = find_available_fonts(size=22) or _default_fonts()
    ctx = _rt.default_context()
    grid_rows, grid_cols, cell_size, padding = 10, 5, size * 2, 4
    grid = torch.full((grid_rows * (cell_size + padding) + padding, grid_cols * (cell_size + padding) + padding), 200, dtype=torch.uint8, device=ctx.device)
    job = Job(size)
    for digit in range(10):
        for _ in range(grid_cols):                            # the preview keeps the discovered font size: no reload, as in the reference
            if digit == 0:
                job.cells.append(_draw_empty_cell(job))
            else:
                _, font = random.choice(fonts)
                job.cells.append(_draw_digit(job, digit, font))
            job.chains.append(_draw_augmentation(size, size, is_empty=(digit == 0)))
    cells = _launch(job, device=True)
    for k in range(grid_rows * grid_cols):
        digit, sample = divmod(k, grid_cols)
        y, x = digit * (cell_size + padding) + padding, sample * (cell_size + padding) + padding
        grid[y:y + cell_size, x:x + cell_size] = ctx.resize_linear(cells[k], (cell_size, cell_size))
    ic.imwrite_png(str(output_path), grid, ctx=ctx)
    print(f"Preview saved to {output_path}")


def main():
    parser = argparse.ArgumentParser(description="Generate synthetic digit dataset (v2)")
    parser.add_argument("--output", "-o", type=Path, default=Path(__file__).parent.parent / "data" / "synthetic_v2", help="Output directory")
    parser.add_argument("--num-per-class", "-n", type=int, default=10000, help="Number of images per class")
    parser.add_argument("--val-ratio", type=float, default=0.1, help="Validation set ratio")
    parser.add_argument("--size", type=int, default=28, help="Image size")
    parser.add_argument("--seed", type=int, default=42, help="Random seed")
    parser.add_argument("--preview", action="store_true", help="Only generate preview image")
    args = parser.parse_args()

    print(f"Output directory: {args.output}")
    if args.preview:
        args.output.mkdir(parents=True, exist_ok=True)
        generate_preview(args.output / "preview.png", args.size)
        return
    print(f"Generating {args.num_per_class} images per class (10 classes)")
    print(f"Total images: {args.num_per_class * 10}")
    print(f"Train/val split: {1 - args.val_ratio:.0%}/{args.val_ratio:.0%}")
    print()
    metadata = generate_dataset(args.output, num_per_class=args.num_per_class, val_ratio=args.val_ratio, size=args.size, seed=args.seed)
    generate_preview(args.output / "preview.png", args.size)
    print()
    print("=" * 50)
    print("Generation complete!")
    print(f"Total images: {metadata['stats']['total_generated']}")
    print(f"Train: {metadata['stats']['train_count']}")
    print(f"Val: {metadata['stats']['val_count']}")
    print(f"Output: {args.output}")
    print("=" * 50)


if __name__ == "__main__":
    main()
