"""No GPU: the restatement of the data set chain (tests/dataset_cells_ref.py) against Pillow, K24's record packing and host check, and the
host-only half of the ml/datasets.py drop-in (names, signatures, weights, CSV handling)."""
import inspect
import io
import os
import sys

import numpy as np
import pytest
import torch

import dataset_cells_ref as R
from dataset_cells_ref import MALFORMED, ML, malformed_records
import png_craft as P

PIL = pytest.importorskip("PIL.Image")


@pytest.fixture(scope="module")
def ds():
    sys.path.insert(0, ML)
    try:
        sys.modules.pop("datasets", None)
        import datasets
        return datasets
    finally:
        sys.path.remove(ML)


@pytest.fixture(scope="module")
def sva():
    import sudoku_vision_amd as sva
    return sva


# ---- the gray decode against Pillow: colour types 0 and 4 at every depth -----------------------------------------------------------------------
@pytest.mark.parametrize("color_type,depth", [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (4, 8), (4, 16)])
def test_gray_decode_against_pillow(color_type, depth):
    s = P.random_samples(9, 13, color_type, depth, seed=3)
    data = P.make_png(s, color_type, depth, filters=[0, 1, 2, 3, 4, 4, 3, 2, 1])
    got, ok = R.gray_decode(data)
    assert ok
    im = PIL.open(io.BytesIO(data))
    if color_type == 4:
        assert im.mode in ("LA", "LA;16B", "RGBA") or depth == 16
        want = s[:, :, 0] >> 8 if depth == 16 else np.asarray(im.convert("LA"))[:, :, 0]
        if depth == 8:
            assert np.array_equal(np.asarray(im)[:, :, 0], s[:, :, 0])
    elif depth == 16:
        assert im.mode.startswith("I;16")
        assert np.array_equal(np.asarray(im).astype(np.int64), s[:, :, 0])      # Pillow keeps 16 bits; cv2's 8-bit read keeps the high byte
        want = s[:, :, 0] >> 8
    elif depth == 1:
        assert im.mode == "1"
        want = np.asarray(im.convert("L"))
    elif depth == 8:
        assert im.mode == "L"
        want = np.asarray(im)
    else:                                                                       # 2 and 4 bits: Pillow opens them as L after bit replication
        want = np.asarray(im.convert("L"))
    assert np.array_equal(got, np.asarray(want).astype(np.uint8))


def test_colour_is_gray_of_bgr():
    import png_decode_ref as D
    import sv_oracle
    s = P.random_samples(7, 5, 6, 8, seed=1)
    data = P.make_png(s, 6, 8, filters=4)
    got, ok = R.gray_decode(data)
    assert ok and np.array_equal(got, sv_oracle.gray(D.decode(data)))


def test_tensor_division_is_torch():
    x = np.arange(256, dtype=np.uint8)
    assert np.array_equal(x.astype(np.float32) / np.float32(255), (torch.from_numpy(x).float() / 255.0).numpy())


# ---- records: packing and sv_dataset_check_records ------------------------------------------------------------------------------------------
def _files():
    out = [P.make_png(P.random_samples(28, 28, 0, 8, seed=1), 0, 8, filters=1), P.make_png(P.random_samples(50, 41, 2, 16, seed=2), 2, 16, filters=4),
           P.make_png(P.random_samples(5, 9, 3, 4, seed=3, limit=7), 3, 4, filters=0, palette=P.random_palette(7)),
           P.make_png(P.random_samples(64, 64, 6, 16, seed=4), 6, 16, filters=3)]
    return out


def test_dataset_pack_records(sva, tmp_path):
    files = _files()
    big = P.make_png(P.random_samples(65, 3, 0, 8), 0, 8)
    lace = P.assemble(4, 4, 0, 8, P.deflate(b"\0" * 20), interlace=1)
    path = tmp_path / "a.png"
    path.write_bytes(files[0])
    packed = sva.host.dataset_pack([str(path), files[1], b"not a png", files[2], big, lace, str(tmp_path / "missing.png"), files[3]], threads=3)
    assert packed.status.tolist() == [0, 0, -1, 0, sva.host.DATASET_TOO_LARGE, -4, -1, 0]
    rec = packed.records
    assert rec.dtype.itemsize == 16 and packed.n == 8 and packed.n_palettes == 1
    import png_decode_ref as D
    buf = packed.pinned.numpy()
    at = 0
    for i, f in zip((0, 1, 3, 7), files):
        h = D.header(f)
        rb = P.row_bytes_of(h["width"], h["type"], h["depth"])
        assert (rec[i]["offset"], rec[i]["width"], rec[i]["height"], rec[i]["color_type"], rec[i]["bit_depth"]) == (at, h["width"], h["height"], h["type"], h["depth"])
        assert rec[i]["palette"] == (0 if h["type"] == 3 else 0xffff)
        import zlib
        n = h["height"] * (1 + rb)
        assert bytes(buf[packed.filtered_at + at:packed.filtered_at + at + n]) == zlib.decompress(h["idat"])
        at += n
    assert packed.filtered_size == at
    for i in (2, 4, 5, 6):
        assert rec[i]["width"] == 0 and rec[i]["height"] == 0
    pal = buf[packed.palettes_at:packed.palettes_at + 1024]
    assert np.array_equal(pal[:21].reshape(7, 3), P.random_palette(7)) and int(pal[768:772].view(np.uint32)[0]) == 7
    good = rec[[0, 1, 3, 7]]
    sva.host.check_dataset_records(good, packed.filtered_size, 1)


def test_check_records(sva):
    base, bad, size = malformed_records(sva)
    sva.host.check_dataset_records(base, size, 3)
    sva.host.check_dataset_records(base, size, 0)
    for name, r in bad.items():
        both = np.concatenate([base, r])
        with pytest.raises(sva._native.NativeError, match="record 1"):
            sva.host.check_dataset_records(both, size, 3)
    with pytest.raises(sva._native.NativeError, match="record 0"):
        sva.host.check_dataset_records(base, size - 1, 3)


# ---- the drop-in's host half ----------------------------------------------------------------------------------------------------------------
REFERENCE_NAMES = {
    "preprocess_cell": ["img"],
    "SyntheticDataset": ["root", "split", "transform"],
    "RealDataset": ["root", "samples", "transform"],
    "get_class_weights": ["dataset", "num_classes"],
    "get_balanced_sampler": ["dataset", "num_classes"],
    "create_combined_dataset": ["synthetic_dir", "real_dir", "split", "transform", "real_weight"],
}
REFERENCE_DEFAULTS = {"SyntheticDataset": {"split": "train", "transform": None}, "RealDataset": {"samples": None, "transform": None},
                      "get_class_weights": {"num_classes": 10}, "get_balanced_sampler": {"num_classes": 10},
                      "create_combined_dataset": {"split": "train", "transform": None, "real_weight": 1.0}}


def test_names_and_signatures(ds):
    for name, params in REFERENCE_NAMES.items():
        obj = getattr(ds, name)
        sig = inspect.signature(obj.__init__ if inspect.isclass(obj) else obj)
        got = [p for p in sig.parameters if p != "self"]
        assert got == params, name
        for k, v in REFERENCE_DEFAULTS.get(name, {}).items():
            assert sig.parameters[k].default == v, (name, k)
    for name in ("Dataset", "ConcatDataset", "WeightedRandomSampler", "Path", "np", "torch"):
        assert hasattr(ds, name)
    assert callable(ds.iterate_batches) and callable(ds.SyntheticDataset.load_batch)


def _tree(root, counts, size=28):
    """root/train/<label>/i.png with counts[label] files each"""
    rs = np.random.RandomState(5)
    for label, k in enumerate(counts):
        if k:
            d = root / "train" / str(label)
            d.mkdir(parents=True)
            for i in range(k):
                PIL.fromarray(rs.randint(0, 256, (size, size), dtype=np.uint8)).save(d / f"{i}.png")


def test_weights_closed_formula(ds, tmp_path, capsys):
    counts = [3, 0, 5, 1, 0, 2, 2, 2, 1, 4]
    _tree(tmp_path, counts)
    syn = ds.SyntheticDataset(tmp_path, "train")
    assert capsys.readouterr().out == "SyntheticDataset (train): 20 samples\n"
    assert len(syn) == 20 and [l for _, l in syn.samples] == sorted(l for _, l in syn.samples)
    w = ds.get_class_weights(syn)
    want = torch.tensor([20 / (10 * c) if c else 0.0 for c in counts], dtype=torch.float32)
    assert w.dtype == torch.float32 and torch.equal(w, want)
    sampler = ds.get_balanced_sampler(syn)
    assert sampler.num_samples == 20 and sampler.replacement
    assert torch.equal(sampler.weights, torch.as_tensor([want[l].item() for _, l in syn.samples], dtype=torch.double))
    cat = ds.ConcatDataset([syn, syn])
    assert torch.equal(ds.get_class_weights(cat), want)
    assert torch.equal(ds.get_class_weights(syn, num_classes=12)[:10], torch.tensor([20 / (12 * c) if c else 0.0 for c in counts], dtype=torch.float32))


def test_real_dataset_csv(ds, tmp_path, capsys):
    rs = np.random.RandomState(6)
    d = tmp_path / "sample_3"
    d.mkdir()
    for name in ("cell_0_0.png", "cell_0_1.png", "cell_0_2.png"):
        PIL.fromarray(rs.randint(0, 256, (50, 50), dtype=np.uint8)).save(d / name)
    (tmp_path / "labels_sample_3.csv").write_text("filename,label\ncell_0_1.png,7\nshort\n\ncell_9_9.png,1\ncell_0_0.png,0,extra\n")
    (tmp_path / "labels_sample_4.csv").write_text("filename,label\ncell_0_0.png,2\n")
    real = ds.RealDataset(tmp_path, samples=["sample_3", "sample_4", "sample_5"])
    out = capsys.readouterr().out
    assert out == f"Warning: {tmp_path / 'sample_4'} not found, skipping\nRealDataset: 2 samples from 3 sources\n"
    assert real.samples == [(d / "cell_0_1.png", 7), (d / "cell_0_0.png", 0)]
    assert len(real) == 2
    both = ds.RealDataset(tmp_path)
    assert sorted(both.samples) == sorted(real.samples)
    with pytest.raises(ValueError, match="No datasets found"):
        ds.create_combined_dataset(tmp_path / "none", tmp_path / "none2")
    comb = ds.create_combined_dataset(tmp_path / "none", tmp_path, real_weight=2.0)
    assert len(comb) == 4 and len(ds.create_combined_dataset(tmp_path, tmp_path, split="val")) == 0
