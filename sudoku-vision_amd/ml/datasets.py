"""MI355X drop-in for the reference's ml/datasets.py: the same names, signatures, defaults, sample order, printed lines and errors.  What the
reference does per sample on one CPU thread -- cv2.imread(path, IMREAD_GRAYSCALE) of a .png, resize to 28x28, CLAHE(2.0, (4,4)),
adaptiveThreshold(GAUSSIAN_C, BINARY, 11, 2), invert, float / 255 (ml/datasets.py:18-46, :69-92, :141-164) -- is here one host pass that
inflates the files on a thread pool (host.dataset_pack) and ONE launch of K24 (csrc/k24_dataset_cells.hip, Context.dataset_cells) for a whole
batch of files, whatever their sizes, colour types and bit depths.

New next to the reference's names: `dataset.load_batch(indices, device=True)` and `iterate_batches(dataset, batch_size, ...)`, which leave the
batch on the GPU for the models and for evaluate_v2.  A file with a side above 64 pixels is read, for that file, through the PNG decoder's gray
read, resize_linear and preprocess_cells: the same arithmetic in more launches.  Colour PNG files: see imgcodecs.imdecode_png(gray=True).
GPU only; there is no CPU fallback.  Not ported: ml/train*.py, tools/dataset_stats.py."""
import os
import sys
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import Dataset, ConcatDataset, WeightedRandomSampler

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bootstrap import package  # noqa: E402
sys.path.pop(0)
_pkg = package()
_rt, _host, _native = _pkg.runtime, _pkg.host, _pkg._native


def _cells_from_images(ctx, imgs):
    """uint8 CUDA tensors [H,W] or [H,W,3] (BGR), sides 1..64 -> (u8 [n,28,28], f32 [n,1,28,28]) of datasets.preprocess_cell, one K24 launch:
    each image becomes the filtered stream of a PNG whose rows all have filter None (a zero byte, then the row; BGR turned to RGB)."""
    rec = np.zeros(len(imgs), _native.DATASET_RECORD_DTYPE)
    rec["palette"] = _native.CELLS_NO_PALETTE
    parts, at = [], 0
    for i, im in enumerate(imgs):
        H, W = int(im.shape[0]), int(im.shape[1])
        rows = im.reshape(H, W) if im.dim() == 2 else im.flip(-1).reshape(H, 3 * W)
        parts.append(torch.cat([torch.zeros((H, 1), dtype=torch.uint8, device=ctx.device), rows], 1).reshape(-1))
        rec[i] = (at, W, H, 0 if im.dim() == 2 else 2, 8, _native.CELLS_NO_PALETTE)
        at += parts[-1].numel()
    n = len(imgs)
    u8 = torch.empty((n, 28, 28), dtype=torch.uint8, device=ctx.device)
    f32 = torch.empty((n, 1, 28, 28), dtype=torch.float32, device=ctx.device)
    status = torch.empty(n, dtype=torch.int32, device=ctx.device)
    ctx.dataset_cells_raw(torch.cat(parts), torch.from_numpy(rec.view(np.uint8)).to(ctx.device), None, _native.CELLS_DATASET, u8, f32, status)
    return u8, f32


def _large_cell(ctx, gray):
    """The composed path for an image K24 does not take (a side above 64): gray u8 CUDA [H,W] -> u8 [28,28]"""
    if tuple(gray.shape) != (28, 28):
        gray = ctx.resize_linear(gray, (28, 28))
    return 255 - ctx.preprocess_cells(gray.reshape(1, 28, 28))[0]


def preprocess_cell(img):
    """Apply consistent preprocessing to cell images (reference ml/datasets.py:18-46): gray if BGR, resize to 28x28, CLAHE, adaptive
    threshold, invert.  img: uint8 [H,W] or [H,W,3], a numpy array (-> numpy) or a CUDA tensor (-> CUDA tensor)."""
    ctx = _rt.default_context(img.device if isinstance(img, torch.Tensor) else None)
    t, was_tensor = _rt._to_dev(img, ctx)
    if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] != 3) or t.numel() == 0:
        raise ValueError(f"preprocess_cell: expected a uint8 image [H,W] or [H,W,3], got {list(t.shape)}")
    if max(t.shape[0], t.shape[1]) <= _native.CELLS_MAX_SIDE:
        out = _cells_from_images(ctx, [t])[0][0]
    else:
        out = _large_cell(ctx, t if t.dim() == 2 else ctx.gray(t[None])[0])
    return _rt._back(out, was_tensor)


def _load_paths(paths, threads=None):
    """Files -> f32 CUDA [n,1,28,28], as the reference's __getitem__ computes each before its transform.  ValueError("Failed to load ...")
    for the first file cv2 could not read (ml/datasets.py:83, :155)."""
    ctx = _rt.default_context()
    packed = _host.dataset_pack([str(p) for p in paths], threads=threads)
    bad = np.nonzero((packed.status != 0) & (packed.status != _host.DATASET_TOO_LARGE))[0]
    if bad.size:
        raise ValueError(f"Failed to load {paths[int(bad[0])]}")
    out = ctx.dataset_cells(packed, "dataset", ("f32",))
    x = out["f32"]
    if packed.n_palettes:                                               # only palette files can fail on the device: cv2 returns None for them
        # bit 0 alone: a file with a side above 64 has a record the kernel refuses (bit 1), and its slot is filled below
        flagged = (out["status"].cpu().numpy() & _native.CELLS_STATUS_PALETTE).nonzero()[0]
        if flagged.size:
            raise ValueError(f"Failed to load {paths[int(flagged[0])]}")
    for i in np.nonzero(packed.status == _host.DATASET_TOO_LARGE)[0]:
        with open(str(paths[int(i)]), "rb") as f:
            data = f.read()
        try:
            gray = ctx.imdecode_png(data, gray=True)
        except _native.NativeError as e:
            if "SV_ERR_BAD_ARG" not in str(e):                          # a malformed file is cv2's None; anything else is not the file's fault
                raise
            raise ValueError(f"Failed to load {paths[int(i)]}") from None
        x[int(i), 0] = _large_cell(ctx, gray).float() / 255.0
    return x


class _CellFiles(Dataset):
    """What the two data sets share: samples = [(path, label)], transform; the reference's __len__ and __getitem__, and load_batch."""

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, idx):
        img_path, label = self.samples[idx]
        tensor = _load_paths([img_path], threads=1)[0].cpu()
        if self.transform:
            tensor = self.transform(tensor)
        return tensor, label

    def load_batch(self, indices, device=True, threads=None):
        """(x f32 [B,1,28,28], labels int64 [B]) of samples[i] for i in indices, from one dataset_pack and one K24 launch; on the GPU unless
        device is False.  transform, when given, is applied to the batch."""
        indices = [int(i) for i in indices]
        x = _load_paths([self.samples[i][0] for i in indices], threads=threads)
        y = torch.tensor([self.samples[i][1] for i in indices], dtype=torch.int64)
        if self.transform:
            x = self.transform(x)
        return (x, y.to(x.device)) if device else (x.cpu(), y)


def _png_files_by_class(split_dir):
    """[(path, label)] of split_dir/<label>/*.png for label 0..9: classes in order, files in the directory's own glob order, a missing
    class directory contributing nothing"""
    found = []
    for digit in range(10):
        folder = split_dir / str(digit)
        if folder.exists():
            found += [(png, digit) for png in folder.glob("*.png")]
    return found


def _labelled_files(csv_path, cell_dir):
    """[(path, label)] of one labels_<sample>.csv, in the file's order.  The first line is the header; a row is `filename,label[,...]`
    split at commas after stripping the line; a row with fewer than two fields, or whose file is not in cell_dir, is passed over."""
    with open(csv_path, "r") as fh:
        rows = [line.strip().split(",") for line in fh.readlines()[1:]]
    named = [(cell_dir / row[0], int(row[1])) for row in rows if len(row) >= 2]
    return [(path, label) for path, label in named if path.exists()]


class SyntheticDataset(_CellFiles):
    """Dataset for synthetic printed digits (reference ml/datasets.py:49-92): root/<split>/<0..9>/*.png, in glob order per class directory."""

    def __init__(self, root: Path, split: str = "train", transform=None):
        self.root = Path(root) / split
        self.transform = transform
        self.samples = _png_files_by_class(self.root)
        print(f"SyntheticDataset ({split}): {len(self.samples)} samples")


class RealDataset(_CellFiles):
    """Dataset for real extracted sudoku cells (reference ml/datasets.py:95-164): root/labels_<sample>.csv (header, then filename,label) beside
    root/<sample>/, in CSV order.  A CSV that is not there is passed over silently, one whose directory is missing with the reference's
    warning; both still count as sources in the printed line."""

    def __init__(self, root: Path, samples: list[str] | None = None, transform=None):
        self.root = Path(root)
        self.transform = transform
        self.samples = []
        sources = list(self.root.glob("labels_*.csv")) if samples is None else [self.root / f"labels_{name}.csv" for name in samples]
        for csv_path in (c for c in sources if c.exists()):
            cell_dir = self.root / csv_path.stem.replace("labels_", "")
            if cell_dir.exists():
                self.samples += _labelled_files(csv_path, cell_dir)
            else:
                print(f"Warning: {cell_dir} not found, skipping")
        print(f"RealDataset: {len(self.samples)} samples from {len(sources)} sources")


def _labels(dataset):
    """Every sample's label in order, without decoding a file where the data set is one of ours (or a ConcatDataset of them)."""
    if isinstance(dataset, _CellFiles):
        return [label for _, label in dataset.samples]
    if isinstance(dataset, ConcatDataset):
        return [label for d in dataset.datasets for label in _labels(d)]
    return [label for _, label in dataset]


def get_class_weights(dataset: Dataset, num_classes: int = 10) -> torch.Tensor:
    """Class weights inversely proportional to class frequency (reference ml/datasets.py:167-185): total / (num_classes * count), 0 for an
    empty class."""
    counts = [0] * num_classes
    for label in _labels(dataset):
        counts[label] += 1
    total = sum(counts)
    weights = [total / (num_classes * c) if c > 0 else 0.0 for c in counts]
    return torch.tensor(weights, dtype=torch.float32)


def get_balanced_sampler(dataset: Dataset, num_classes: int = 10) -> WeightedRandomSampler:
    """A sampler that balances classes during training (reference ml/datasets.py:188-201)."""
    class_weights = get_class_weights(dataset, num_classes)
    sample_weights = [class_weights[label].item() for label in _labels(dataset)]
    return WeightedRandomSampler(weights=sample_weights, num_samples=len(dataset), replacement=True)


def create_combined_dataset(
    synthetic_dir: Path,
    real_dir: Path,
    split: str = "train",
    transform=None,
    real_weight: float = 1.0,
) -> Dataset:
    """Synthetic data plus, for split "train", the real data int(real_weight) times (reference ml/datasets.py:204-243)."""
    synthetic_dir, real_dir = Path(synthetic_dir), Path(real_dir)
    parts = [SyntheticDataset(synthetic_dir, split=split, transform=transform)] if synthetic_dir.exists() else []
    if split == "train" and real_dir.exists():                          # real cells only train; the SAME object int(real_weight) times
        parts += [RealDataset(real_dir, transform=transform)] * int(real_weight)
    if not parts:
        raise ValueError("No datasets found")
    return ConcatDataset(parts)


def _resolve(dataset, idx):
    """index -> (the _CellFiles data set that owns it, its index there)"""
    if isinstance(dataset, ConcatDataset):
        if idx < 0 or idx >= len(dataset):
            raise IndexError(idx)
        k = int(np.searchsorted(dataset.cumulative_sizes, idx, side="right"))
        return _resolve(dataset.datasets[k], idx - (dataset.cumulative_sizes[k - 1] if k else 0))
    if not isinstance(dataset, _CellFiles):
        raise TypeError("iterate_batches takes a SyntheticDataset, a RealDataset or a ConcatDataset of them")
    return dataset, idx


def iterate_batches(dataset, batch_size, shuffle=False, sampler=None, threads=None):
    """A generator of (x f32 [B,1,28,28], labels int64 [B]) batches on the GPU over `dataset` (one of the two classes here or a ConcatDataset
    of them): the loader of evaluate_v2.evaluate_dataset / evaluate, without a host round trip of the images.  Order: the sampler's, a random
    permutation (shuffle) or 0 .. len - 1.  Each data set's transform is applied to its samples of the batch."""
    if sampler is not None:
        order = [int(i) for i in sampler]
    elif shuffle:
        order = torch.randperm(len(dataset)).tolist()
    else:
        order = list(range(len(dataset)))
    for at in range(0, len(order), int(batch_size)):
        owners = [_resolve(dataset, i) for i in order[at:at + int(batch_size)]]
        x = _load_paths([d.samples[i][0] for d, i in owners], threads=threads)
        y = torch.tensor([d.samples[i][1] for d, i in owners], dtype=torch.int64, device=x.device)
        for d in {id(d): d for d, _ in owners}.values():
            if d.transform:
                rows = torch.tensor([k for k, (o, _) in enumerate(owners) if o is d], device=x.device)
                x[rows] = d.transform(x[rows])
        yield x, y
