"""GPU (-m gpu): K24 (sv_dataset_cells), the gray PNG read and the ml/datasets.py drop-in, bit-exact on out_u8 and out_f32 against the
restatement of the reference's chain (tests/dataset_cells_ref.py).  Shapes are the smallest at which the kernel can still go wrong: every filter,
first rows with nothing above, the 512-byte row cap, 1-pixel sides, partial last bytes, both LDS classes in one batch of 67."""
import io
import os
import sys

import numpy as np
import pytest
import torch

import dataset_cells_ref as R
import png_craft as P
import png_decode_ref as D
from dataset_cells_ref import MALFORMED, ML, malformed_records

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sva():
    import sudoku_vision_amd as sva
    return sva


def _gray28(seed):
    return P.random_samples(28, 28, 0, 8, seed=seed)


def _case_files():
    """name -> file bytes: the issue's list"""
    f = {}
    for k in range(5):
        f[f"28x28 filter {k}"] = P.make_png(_gray28(k), 0, 8, filters=k)
    f["28x28 filters cycling"] = P.make_png(_gray28(7), 0, 8, filters=[r % 5 for r in range(28)])
    f["28x28 first row Up"] = P.make_png(_gray28(8), 0, 8, filters=[2] + [1] * 27)
    f["28x28 first row Paeth"] = P.make_png(_gray28(9), 0, 8, filters=[4] + [3] * 27)
    f["1x1"] = P.make_png(P.random_samples(1, 1, 0, 8, seed=1), 0, 8, filters=4)
    f["64x64 RGBA16"] = P.make_png(P.random_samples(64, 64, 6, 16, seed=2), 6, 16, filters=[(r * 3) % 5 for r in range(64)])
    f["64x1"] = P.make_png(P.random_samples(1, 64, 0, 8, seed=3), 0, 8, filters=1)
    f["1x64"] = P.make_png(P.random_samples(64, 1, 0, 8, seed=4), 0, 8, filters=[r % 5 for r in range(64)])
    f["63x64 Paeth"] = P.make_png(P.random_samples(64, 63, 0, 8, seed=5), 0, 8, filters=4)
    f["29x27"] = P.make_png(P.random_samples(27, 29, 0, 8, seed=6), 0, 8, filters=3)
    f["50x50"] = P.make_png(P.random_samples(50, 50, 0, 8, seed=7), 0, 8, filters=[r % 5 for r in range(50)])
    f["9x5 1 bit"] = P.make_png(P.random_samples(5, 9, 0, 1, seed=8), 0, 1, filters=[0, 1, 2, 3, 4])
    f["5x5 2 bits"] = P.make_png(P.random_samples(5, 5, 0, 2, seed=9), 0, 2, filters=2)
    f["5x5 4 bits"] = P.make_png(P.random_samples(5, 5, 0, 4, seed=10), 0, 4, filters=4)
    for t, d in ((2, 8), (2, 16), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)):
        pal = P.random_palette(200, seed=t) if t == 3 else None
        f[f"type {t} depth {d}"] = P.make_png(P.random_samples(30, 33, t, d, seed=t + d, limit=200 if t == 3 else None), t, d, filters=[r % 5 for r in range(30)], palette=pal)
    for v in (0, 128, 255):
        f[f"constant {v}"] = P.make_png(np.full((28, 28, 1), v), 0, 8, filters=1)
    return f


FILES = _case_files()
_REF = {}


def ref(name, mode):
    if (name, mode) not in _REF:
        _REF[name, mode] = R.cell(FILES[name], mode)
    return _REF[name, mode]


def run(ctx, sva, datas, mode, want=("u8", "f32")):
    packed = sva.host.dataset_pack(datas, threads=4)
    assert not packed.status.any()
    out = ctx.dataset_cells(packed, mode, want)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("mode", ["gray", "dataset"])
@pytest.mark.parametrize("name", list(FILES))
def test_single_cells(ctx, sva, name, mode):
    out = run(ctx, sva, [FILES[name]], mode)
    u8, f32, ok = ref(name, mode)
    assert ok and out["status"][0] == 0
    assert np.array_equal(out["u8"][0], u8), name
    assert out["f32"].dtype == np.float32 and np.array_equal(out["f32"][0, 0].view(np.uint32), f32.view(np.uint32)), name


def test_batch_of_67_and_permutation(ctx, sva):
    names = (list(FILES) * 3)[:67]
    out = run(ctx, sva, [FILES[n] for n in names], "dataset")
    for i, n in enumerate(names):
        u8, f32, _ = ref(n, "dataset")
        assert np.array_equal(out["u8"][i], u8) and np.array_equal(out["f32"][i, 0], f32), (i, n)
    assert not out["status"].any()
    perm = np.random.RandomState(1).permutation(67)
    again = run(ctx, sva, [FILES[names[j]] for j in perm], "dataset")
    assert np.array_equal(again["u8"], out["u8"][perm]) and np.array_equal(again["f32"], out["f32"][perm])


def test_palette_index_past_the_end(ctx, sva):
    s = P.random_samples(28, 28, 3, 8, seed=3, limit=10)
    s[5, 6, 0] = 10
    bad = P.make_png(s, 3, 8, filters=1, palette=P.random_palette(10))
    names = ["28x28 filter 1", "type 3 depth 8", "50x50"]
    datas = [FILES[names[0]], bad, FILES[names[1]], FILES[names[2]]]
    out = run(ctx, sva, datas, "gray")
    assert out["status"].tolist() == [0, 1, 0, 0]
    u8, _, ok = R.cell(bad, "gray")
    assert not ok and u8[5, 6] == 0 and np.array_equal(out["u8"][1], u8)
    for i, n in zip((0, 2, 3), names):
        assert np.array_equal(out["u8"][i], ref(n, "gray")[0])


def test_refused_records(ctx, sva):
    """Records sv_dataset_check_records refuses, handed to the kernel: refused cells are zeros with bit 1, neighbours exact."""
    base, bad, size = malformed_records(sva)
    h = D.header(FILES["28x28 filter 4"])
    import zlib
    filtered = np.frombuffer(zlib.decompress(h["idat"]), np.uint8)
    assert filtered.size == size
    rec = np.concatenate(sum(([r, base] for r in bad.values()), [base]))
    n = rec.size
    dev = lambda a: torch.from_numpy(np.array(a)).to(ctx.device)
    pal = np.zeros(3 * 1024, np.uint8)
    u8 = torch.full((n, 28, 28), 7, dtype=torch.uint8, device=ctx.device)
    f32 = torch.full((n, 1, 28, 28), 7.0, device=ctx.device)
    status = torch.full((n,), -1, dtype=torch.int32, device=ctx.device)
    ctx.dataset_cells_raw(dev(filtered), dev(rec.view(np.uint8)), dev(pal), sva._native.CELLS_DATASET, u8, f32, status)
    torch.cuda.synchronize()
    want_u8, want_f32, _ = ref("28x28 filter 4", "dataset")
    st = status.cpu().numpy()
    for i in range(n):
        if i % 2 == 0:
            assert st[i] == 0 and np.array_equal(u8[i].cpu().numpy(), want_u8) and np.array_equal(f32[i, 0].cpu().numpy(), want_f32), i
        else:
            assert st[i] == 2 and not u8[i].any() and not f32[i].any(), (i, list(MALFORMED)[i // 2])
    assert n == 2 * len(MALFORMED) + 1


@pytest.mark.parametrize("want", [("u8",), ("f32",), ("u8", "f32")])
def test_outputs_wanted(ctx, sva, want):
    out = run(ctx, sva, [FILES["50x50"], FILES["28x28 filter 3"]], "dataset", want)
    assert set(out) == set(want) | {"status"}
    for i, n in enumerate(("50x50", "28x28 filter 3")):
        u8, f32, _ = ref(n, "dataset")
        if "u8" in want:
            assert np.array_equal(out["u8"][i], u8)
        if "f32" in want:
            assert np.array_equal(out["f32"][i, 0], f32)


def _side_stream():
    """A side stream that leaves the modules run after this one the streams they get without it.  torch hands out streams from a pool of 32
    in turn, and HIP spreads streams over a few hardware queues (4 by default) in their order: taking ONE stream here moves the side stream
    of every later module to the next queue, and tests/test_gpu_stream_order.py's controls then find theirs on the default stream's queue,
    where the default stream waits behind the delay ("control count_nonzero saw B", in a whole-suite run only).  So a whole turn of the pool
    is taken: the first stream is used, and the next module is handed that same one again."""
    s = torch.cuda.Stream()
    for _ in range(31):
        torch.cuda.Stream()
    return s


def test_side_stream_and_graph_replay(ctx, sva):
    """The call on a busy side stream sees the bytes copied behind the delay; captured once and replayed twice, status is written anew each time."""
    names = ["50x50", "28x28 filter 4", "64x64 RGBA16"]
    pa = sva.host.dataset_pack([FILES[n] for n in names])
    pb = sva.host.dataset_pack([FILES[n] for n in reversed(names)])
    assert pa.pinned.numel() == pb.pinned.numel()
    n = 3
    A, B = pa.pinned.to(ctx.device), pb.pinned.to(ctx.device)
    buf = A.clone()
    u8 = torch.empty((n, 28, 28), dtype=torch.uint8, device=ctx.device)
    f32 = torch.empty((n, 1, 28, 28), dtype=torch.float32, device=ctx.device)
    status = torch.empty(n, dtype=torch.int32, device=ctx.device)
    call = lambda: ctx.dataset_cells_raw(buf[pa.filtered_at:pa.filtered_at + pa.filtered_size], buf[:16 * n], None, sva._native.CELLS_DATASET, u8, f32, status)
    want = lambda order: np.stack([ref(k, "dataset")[0] for k in order])
    s = _side_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call()
        s.synchronize()
        assert np.array_equal(u8.cpu().numpy(), want(names))
        torch.cuda._sleep(20_000_000)
        buf.copy_(B, non_blocking=True)
        call()
    s.synchronize()
    assert np.array_equal(u8.cpu().numpy(), want(names[::-1])) and not status.cpu().numpy().any()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s, capture_error_mode="global"):
            call()
        for src, order in ((A, names), (B, names[::-1])):
            buf.copy_(src)
            status.fill_(3)
            u8.zero_()
            g.replay()
            s.synchronize()
            assert np.array_equal(u8.cpu().numpy(), want(order)) and not status.cpu().numpy().any()
            assert np.array_equal(f32.cpu().numpy()[:, 0], np.stack([ref(k, "dataset")[1] for k in order]))


# ---- the gray read of the PNG decoder ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color_type,depth", [(0, 8), (0, 1), (0, 16), (2, 8), (3, 4), (4, 16), (6, 8)])
def test_imdecode_png_gray(ctx, sva, color_type, depth, tmp_path):
    from sudoku_vision_amd import imgcodecs as ic
    pal = P.random_palette(16) if color_type == 3 else None
    s = P.random_samples(3, 257, color_type, depth, seed=2, limit=16 if color_type == 3 else None)
    data = P.make_png(s, color_type, depth, filters=[1, 4, 3], palette=pal)
    want, ok = R.gray_decode(data)
    assert ok
    got = ic.imdecode_png(data, gray=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    dev = ic.imdecode_png(data, device=True, gray=True)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)
    path = tmp_path / "x.png"
    path.write_bytes(data)
    assert np.array_equal(ic.imread_png(str(path), gray=True), want)
    assert np.array_equal(ic.imread_png(str(path)), D.decode(data)) and np.array_equal(ic.imdecode_png(data), D.decode(data))
    wide = torch.zeros((2, 3, 300), dtype=torch.uint8, device=ctx.device)
    out = ctx.imdecode_png_batch([data, data], out=wide[:, :, :257], gray=True)
    torch.cuda.synchronize()
    assert np.array_equal(out[1].cpu().numpy(), want) and not wide[:, :, 257:].any()


# ---- the drop-in ------------------------------------------------------------------------------------------------------------------------------
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
def tree(tmp_path_factory, ds):
    PIL = pytest.importorskip("PIL.Image")
    root = tmp_path_factory.mktemp("cells")
    rs = np.random.RandomState(11)
    for label, k in enumerate([3, 0, 4, 2, 0, 3, 2, 3, 2, 3]):
        if k:
            d = root / "syn" / "train" / str(label)
            d.mkdir(parents=True)
            for i in range(k):
                PIL.fromarray(rs.randint(0, 256, (28, 28), dtype=np.uint8)).save(d / f"{i}.png")
    d = root / "real" / "sample_1"
    d.mkdir(parents=True)
    lines = ["filename,label"]
    for i in range(18):
        side = 50 if i % 2 else 28
        PIL.fromarray(rs.randint(0, 256, (side, side), dtype=np.uint8)).save(d / f"cell_{i}.png")
        lines.append(f"cell_{i}.png,{i % 10}")
    (root / "real" / "labels_sample_1.csv").write_text("\n".join(lines) + "\n")
    return ds.SyntheticDataset(root / "syn"), ds.RealDataset(root / "real")


def _want(path):
    with open(path, "rb") as f:
        return R.cell(f.read(), "dataset")[1]


def test_dropin_getitem_and_load_batch(ds, tree):
    syn, real = tree
    assert len(syn) == 22 and len(real) == 18
    for d in (syn, real):
        x, y = d.load_batch(range(len(d)))
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (len(d), 1, 28, 28) and y.dtype == torch.int64 and y.is_cuda
        assert y.tolist() == [l for _, l in d.samples]
        for i in range(len(d)):
            t, label = d[i]
            assert not t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (1, 28, 28) and label == d.samples[i][1] and isinstance(label, int)
            assert np.array_equal(t[0].numpy(), _want(d.samples[i][0])) and torch.equal(x[i].cpu(), t)
        for i in range(len(d)):
            assert np.array_equal(x[i, 0].cpu().numpy(), _want(d.samples[i][0])), i


def test_dropin_iterate_batches_and_evaluate(ds, tree, ctx):
    syn, real = tree
    cat = ds.ConcatDataset([syn, real, real])
    xs, ys = [], []
    for x, y in ds.iterate_batches(cat, 16):
        assert x.is_cuda and y.is_cuda and x.shape[0] <= 16
        xs.append(x)
        ys.append(y)
    x, y = torch.cat(xs), torch.cat(ys)
    assert x.shape[0] == len(cat) == 58 and [len(b) for b in xs] == [16, 16, 16, 10]
    paths = [p for p, _ in syn.samples + real.samples + real.samples]
    assert y.tolist() == [l for _, l in syn.samples + real.samples + real.samples]
    for i in (0, 21, 22, 39, 40, 57):
        assert np.array_equal(x[i, 0].cpu().numpy(), _want(paths[i])), i
    sys.path.insert(0, ML)
    try:
        for name in ("evaluate_v2", "model"):
            sys.modules.pop(name, None)
        import evaluate_v2 as ev
        from model import DigitCNN
    finally:
        sys.path.remove(ML)
    import cnn_oracle
    model = DigitCNN()
    model.load_state_dict({k: torch.as_tensor(v) for k, v in cnn_oracle.random_state_dict(1234).items()})
    model = model.to(ctx.device).eval()
    res = ev.evaluate_dataset(model, ds.iterate_batches(cat, 16), ctx.device, "cells")
    assert res["samples"] == 58
    with torch.no_grad():
        pred = model(x).argmax(1)
    assert res["accuracy"] == pytest.approx(float((pred == y).float().mean()))


@pytest.mark.parametrize("shape", [(28, 28), (50, 50), (33, 40, 3)])
def test_dropin_preprocess_cell(ds, ctx, shape):
    import sv_oracle
    img = np.random.RandomState(sum(shape)).randint(0, 256, shape, dtype=np.uint8)
    want = R.cell_of_gray(img if img.ndim == 2 else sv_oracle.gray(img), "dataset")[0]
    got = ds.preprocess_cell(img)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    t = ds.preprocess_cell(torch.from_numpy(img).to(ctx.device))
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), want)


def test_dropin_files_above_64(ds, ctx, tmp_path):
    """A file with a side above 64 is not K24's: its slot is filled through the PNG decoder's gray read, resize_linear and preprocess_cells.
    Alone (a pack without one decodable file), beside small files, and beside a palette file, whose presence makes the loader read the
    device status: the large file's refused record must not be taken for a failed file."""
    files = {"0/a_65x40.png": P.make_png(P.random_samples(40, 65, 0, 8, seed=1), 0, 8, filters=[r % 5 for r in range(40)]),
             "1/b_100x100.png": P.make_png(P.random_samples(100, 100, 0, 8, seed=2), 0, 8, filters=4),
             "2/c_palette.png": P.make_png(P.random_samples(28, 28, 3, 8, seed=3, limit=9), 3, 8, filters=1, palette=P.random_palette(9)),
             "3/d_28x28.png": FILES["28x28 filter 2"],
             "4/e_70x90_rgb.png": P.make_png(P.random_samples(90, 70, 2, 8, seed=4), 2, 8, filters=3)}
    for name, data in files.items():
        (tmp_path / "train" / name).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / "train" / name).write_bytes(data)
    syn = ds.SyntheticDataset(tmp_path)
    assert [p.name for p, _ in syn.samples] == [n.split("/")[1] for n in files]
    want = [R.cell(data, "dataset")[1] for data in files.values()]
    for i in range(5):                                                  # alone: indices 0, 1 and 4 are packs with nothing K24 decodes
        t, label = syn[i]
        assert label == i and np.array_equal(t[0].numpy(), want[i]), i
    for idx in ([0, 1], [0, 3, 1], [2, 0], [0, 1, 2, 3, 4], [4, 2, 1, 3, 0, 2]):
        x, y = syn.load_batch(idx)
        assert y.tolist() == idx
        for k, i in enumerate(idx):
            assert np.array_equal(x[k, 0].cpu().numpy(), want[i]), (idx, k)
    got = torch.cat([x for x, _ in ds.iterate_batches(ds.ConcatDataset([syn, syn]), 4)])
    assert np.array_equal(got[:, 0].cpu().numpy(), np.stack(want + want))
    s = P.random_samples(28, 28, 3, 8, seed=5, limit=9)
    s[0, 0, 0] = 9                                                      # past the palette's end: cv2 returns None, whatever else the batch holds
    (tmp_path / "train" / "2" / "c_palette.png").write_bytes(P.make_png(s, 3, 8, filters=1, palette=P.random_palette(9)))
    with pytest.raises(ValueError, match="Failed to load .*c_palette.png"):
        syn.load_batch([0, 2, 1])


@pytest.mark.parametrize("shape", [(40, 65), (100, 100), (90, 70, 3)])
def test_dropin_preprocess_cell_above_64(ds, ctx, shape):
    import sv_oracle
    img = np.random.RandomState(sum(shape)).randint(0, 256, shape, dtype=np.uint8)
    want = R.cell_of_gray(img if img.ndim == 2 else sv_oracle.gray(img), "dataset")[0]
    got = ds.preprocess_cell(img)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    t = ds.preprocess_cell(torch.from_numpy(img).to(ctx.device))
    assert t.is_cuda and tuple(t.shape) == (28, 28) and np.array_equal(t.cpu().numpy(), want)


def test_timing_tool_smoke(ctx, monkeypatch, tmp_path):
    """tools/time_dataset_cells.py --smoke: every column is there and finite, and its own check that the composed path equals K24 holds."""
    import importlib
    import json
    monkeypatch.setattr(sys, "path", list(sys.path))                   # the tool puts its own directories in front: undone after the test
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(ML), "..", "tools"))
    out = tmp_path / "t.json"
    monkeypatch.setattr(sys, "argv", ["time_dataset_cells.py", "--smoke", "--json", str(out)])
    sys.modules.pop("datasets", None)
    tool = importlib.import_module("time_dataset_cells")
    res = tool.main()
    assert json.loads(out.read_text())["rows"] == json.loads(json.dumps(res))["rows"]
    assert [r["cells"] for r in res["rows"]] == [64, 128, 16]
    for r in res["rows"]:
        for k in ("k24_launch", "device_copy_of_the_same_bytes", "composed_k19_gray_resize_preprocess_torch"):
            assert np.isfinite(r[k]["median_ms"]) and r[k]["median_ms"] > 0
        assert r["hbm_floor_ms"] > 0
    assert res["host"]["files"] == 128 and res["end_to_end"]["files"] == 128 and res["end_to_end"]["iterate_batches_wall"]["median_ms"] > 0
