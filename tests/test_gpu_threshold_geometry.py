"""GPU (-m gpu): every K1 kernel against tests/threshold_ref.py (itself bit-exact with the C oracle, tests/test_threshold_ref.py) at
the shapes, layouts and contents where its launch regimes change: k_preprocess_any, k_preprocess_f32 (unaligned width, a 3-byte
offset view, a pitch not a multiple of 4), k_preprocess_march<false|true> (last strip widths, one band, short last bands, the
batch-driven band heights at 1080p), k_preprocess_warp_fused, the test-only matrix-pipe k_preprocess_mm (exact re-decision and
its take-every-pixel path), the stand-alone k_gray (all 2^24 colours), k_blur and k_adaptive_threshold (every block and C), and
N1's k_preprocess_cells.  Batches mix contents frame by frame (tie-dense, noise, flat, all-0, all-255, grid, ...).  Batches over
16 frames are compared frame by frame with the C oracle and on a sample with the restatement.

Only device tensors of the expected dtype reach a Context method here; every view stays inside its allocation."""
from dataclasses import dataclass
import functools
import os

import numpy as np
import pytest
import torch

import cnn_oracle
import sv_oracle as o
import threshold_ref as T
from sudoku_vision_amd import _native
from sudoku_vision_amd.runtime import Context

pytestmark = pytest.mark.gpu

MARCH_STRIP = 240          # k1_threshold.hip: output columns per marching wave


def march_shape(n, H, W):
    """Mirror of march_shape() in k1_threshold.hip (geometry only) -> (nstrips, nbands, band height TH)."""
    nstrips = (W + MARCH_STRIP - 1) // MARCH_STRIP
    nbands = (12288 + n * nstrips - 1) // (n * nstrips)
    nbands = max(1, min(nbands, H // 32))
    TH = (H + nbands - 1) // nbands
    return nstrips, (H + TH - 1) // TH, TH


def regime(n, H, W, layout):
    """Mirror of the launch choice in svk_preprocess: which kernel a preprocess() call of this geometry runs."""
    if H < 16 or W < 16:
        return "any"
    if layout != "dense" or W % 4:
        return "f32"
    return "march"


@dataclass
class Shape:
    name: str
    n: int
    H: int
    W: int
    layout: str = "dense"        # "dense", "crop3" (a column-cropped view 3 bytes off), "pitch" (row pitch not a multiple of 4)
    contents: tuple = ("tie", "noise")

    @property
    def regime(self):
        return regime(self.n, self.H, self.W, self.layout)

    @property
    def march(self):
        nstrips, nbands, TH = march_shape(self.n, self.H, self.W)
        last_strip = self.W - (nstrips - 1) * MARCH_STRIP
        return {"nstrips": nstrips, "nbands": nbands, "TH": TH, "last_band": self.H - (nbands - 1) * TH, "last_strip": last_strip}


MIX = T.CONTENTS
SHAPES = [
    # k_preprocess_any: H < 16 or W < 16
    Shape("any_1x1", 3, 1, 1, contents=("noise", "zeros", "full")),
    Shape("any_1x1920", 2, 1, 1920), Shape("any_15x1000", 2, 15, 1000), Shape("any_1080x1", 2, 1080, 1),
    Shape("any_1080x15", 2, 1080, 15), Shape("any_15x15", 3, 15, 15, contents=("tie", "noise", "grid")),
    # k_preprocess_f32: W % 4 != 0, a 3-byte offset, an odd pitch; tile edges at 64k +- 1
    Shape("f32_65x65", 2, 65, 65), Shape("f32_64x129", 2, 64, 129), Shape("f32_63x127", 2, 63, 127), Shape("f32_129x193", 2, 129, 193),
    Shape("f32_1079x1919", 1, 1079, 1919, contents=("tie",)),
    Shape("f32_crop3_64x128", 2, 64, 128, "crop3"), Shape("f32_crop3_97x244", 2, 97, 244, "crop3"),
    Shape("f32_pitch_64x128", 2, 64, 128, "pitch"), Shape("f32_pitch_130x480", 2, 130, 480, "pitch"),
    # k_preprocess_march<false>: last strip 4 / 16 / 236 / 240 columns, both edges in one wave, one band, short last bands
    Shape("march_40x244", 2, 40, 244), Shape("march_70x256", 2, 70, 256), Shape("march_70x476", 2, 70, 476),
    Shape("march_70x480", 2, 70, 480), Shape("march_16x16", 2, 16, 16), Shape("march_20x20", 2, 20, 20),
    Shape("march_7x200x484", 7, 200, 484, contents=MIX[:7]), Shape("march_83x97x1000", 83, 97, 1000, contents=MIX),
    Shape("march_1080p_n1", 1, 1080, 1920, contents=("tie",)), Shape("march_1080p_n64", 64, 1080, 1920, contents=MIX),
    Shape("march_1080p_n256", 256, 1080, 1920, contents=MIX),
]
BY_NAME = {s.name: s for s in SHAPES}


def test_shape_table_reaches_every_regime():
    reg = {s.regime for s in SHAPES}
    assert reg == {"any", "f32", "march"}
    f32 = [s for s in SHAPES if s.regime == "f32"]
    assert {s.layout for s in f32} == {"dense", "crop3", "pitch"} and any(s.W % 4 for s in f32)
    assert any(s.W % 64 in (1, 63) for s in f32) and any(s.H % 64 in (1, 63) for s in f32)
    march = [s.march for s in SHAPES if s.regime == "march"]
    assert {4, 16, 236, 240} <= {m["last_strip"] for m in march}
    assert any(m["nstrips"] == 1 and s.W <= 256 - 16 for m, s in zip(march, [s for s in SHAPES if s.regime == "march"]))
    assert any(m["nbands"] == 1 for m in march)
    assert any(m["nbands"] > 1 and m["last_band"] < m["TH"] for m in march)
    assert BY_NAME["march_7x200x484"].march == {"nstrips": 3, "nbands": 6, "TH": 34, "last_band": 30, "last_strip": 4}
    assert BY_NAME["march_83x97x1000"].march["nbands"] == 3 and BY_NAME["march_83x97x1000"].march["last_band"] == 31
    assert [BY_NAME[f"march_1080p_n{n}"].march["nbands"] for n in (1, 64, 256)] == [33, 24, 6]
    assert [BY_NAME[f"march_1080p_n{n}"].march["TH"] for n in (64, 256)] == [45, 180]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _content(kind, H, W, seed):
    return T.content_frame(kind, H, W, seed)


def _distinct(s):
    """The distinct frames of shape s: one per content kind (frame f of the batch is distinct[f % len])."""
    return [_content(k, s.H, s.W, i) for i, k in enumerate(s.contents)]


def _device_batch(s, distinct):
    """Frames u8 [n, H, W, 3] on the device in s.layout, and the dense copy."""
    d = _dev(np.stack(distinct))
    dense = d[torch.arange(s.n, device="cuda") % len(distinct)].contiguous()
    if s.layout == "dense":
        return dense, dense
    g = torch.Generator(device="cuda").manual_seed(s.H * s.W)
    if s.layout == "crop3":                            # frames[:, :, 1:] of one column more: data pointer 3 bytes off
        buf = torch.randint(0, 256, (s.n, s.H, s.W + 1, 3), dtype=torch.uint8, device="cuda", generator=g)
        view = buf[:, :, 1:]
        assert view.data_ptr() % 4 == 3
    else:                                              # rows padded so that the pitch is not a multiple of 4
        pitch = 3 * s.W + (2 if (3 * s.W + 2) % 4 else 1)
        buf = torch.randint(0, 256, (s.n * s.H * pitch,), dtype=torch.uint8, device="cuda", generator=g)
        view = torch.as_strided(buf, (s.n, s.H, s.W, 3), (s.H * pitch, pitch, 3, 1))
        assert pitch % 4
    view.copy_(dense)
    return view, dense


def _report(got, want, what, frame=None):
    """Bit-exact, or an assertion naming the first mismatching pixel and, for a BGR frame, its f32 mean from the restatement."""
    bad = np.argwhere(got != want)
    if bad.size:
        p = tuple(bad[0])
        info = ""
        if frame is not None:
            b, m, _ = T.preprocess_parts(frame)
            info = f"; blurred src {b[p]}, f32 mean {float(m[p])!r} (tie at src + 1.5 = {b[p] + 1.5})"
        raise AssertionError(f"{what}: {len(bad)} mismatches, first at {p}: got {got[p]} want {want[p]}{info}")


@pytest.mark.parametrize("s", SHAPES, ids=lambda s: s.name)
def test_preprocess(ctx, s):
    distinct = _distinct(s)
    view, dense = _device_batch(s, distinct)
    got = ctx.preprocess(view)
    wants = [_dev(o.preprocess_for_grid_detection(f)) for f in distinct]
    for f in range(s.n):                               # every frame against the C oracle
        w = wants[f % len(distinct)]
        if not torch.equal(got[f], w):
            _report(got[f].cpu().numpy(), w.cpu().numpy(), f"{s.name} frame {f} vs oracle", distinct[f % len(distinct)])
    sample = range(len(distinct)) if s.n * s.H * s.W <= 16 * 1080 * 1920 // 8 else range(min(2, len(distinct)))
    for i in sample:                                   # and the restatement, which names the f32 mean of a mismatch
        _report(got[i].cpu().numpy(), T.preprocess(distinct[i]), f"{s.name} frame {i} vs threshold_ref", distinct[i])
    if s.layout != "dense":
        assert torch.equal(got, ctx.preprocess(dense))


BITS = [(H, W, n) for W in (32, 256, 480, 736, 1920) for n in (1, 7) for H in (40,)]


@pytest.mark.parametrize("H,W,n", BITS, ids=lambda v: str(v))
def test_preprocess_bits(ctx, H, W, n):
    s = Shape(f"bits_{W}_{n}", n, H, W, contents=MIX[:n] if n > 1 else ("tie",))
    distinct = _distinct(s)
    dense, _ = _device_batch(s, distinct)
    bits = ctx.preprocess_bits(dense).cpu().numpy()
    got = np.unpackbits(bits.view(np.uint8).reshape(n, H, -1), axis=2, bitorder="little").astype(np.uint8) * 255
    for f in range(n):
        fr = distinct[f % len(distinct)]
        _report(got[f], o.preprocess_for_grid_detection(fr), f"bits W={W} n={n} frame {f}", fr)
    _report(got[0], T.preprocess(distinct[0]), f"bits W={W} vs threshold_ref", distinct[0])


@pytest.mark.parametrize("n", [1, 7, 9, 17])
def test_preprocess_warp_fused(ctx, n):
    s = Shape(f"fused_{n}", n, 96, 160, contents=MIX)
    distinct = _distinct(s)
    dense, _ = _device_batch(s, distinct)
    corners = np.tile(np.array([[12, 9], [150, 14], [146, 90], [8, 84]], np.float32), (n, 1, 1))
    corners += np.arange(n, dtype=np.float32)[:, None, None] % 3
    minv = ctx.minv_to_device(Context.corners_to_minv(corners))
    binary, cells = ctx.preprocess_and_warp_cells(dense, minv)
    assert torch.equal(cells, ctx.warp_cells(dense, minv))
    for f in range(n):
        fr = distinct[f % len(distinct)]
        _report(binary[f].cpu().numpy(), o.preprocess_for_grid_detection(fr), f"warp_fused n={n} frame {f}", fr)
    _report(binary[0].cpu().numpy(), T.preprocess(distinct[0]), f"warp_fused n={n} vs threshold_ref", distinct[0])


def test_matrix_pipe_form(ctx):
    """k_preprocess_mm (test-only library) on tie-dense frames, where the approximate mean cannot decide and the exact re-decision
    runs, and on the stripes frame, whose interior 64 x 128 tiles have more than 1/8 of their pixels ambiguous: every pixel of
    such a tile is re-decided."""
    xc = Context(library=_native.lib_xcheck())
    frames = np.stack([T.tie_frame(128, 256, 3), T.stripes_frame(128, 256), T.content_frame("noise", 128, 256, 4)])
    d = _dev(frames)
    for i in (0, 1, 2):
        xc.preprocess_stats()                                    # switches the counter on / resets it
        got = xc.preprocess_mm(d[i:i + 1])
        redecided, _ = xc.preprocess_stats()
        _report(got[0].cpu().numpy(), o.preprocess_for_grid_detection(frames[i]), f"mm frame {i}", frames[i])
        _report(got[0].cpu().numpy(), T.preprocess(frames[i]), f"mm frame {i} vs threshold_ref", frames[i])
        if i == 0:
            assert redecided >= 20, redecided                    # the tie patches' centres at least
        if i == 1:
            assert redecided >= 64 * 128, redecided              # a whole tile re-decided
    assert torch.equal(xc.preprocess_mm(d), ctx.preprocess(d))


# ---- stand-alone stages -----------------------------------------------------------------------------------------------------------
def test_gray_all_colours(ctx):
    """k_gray on all 2^24 BGR triples as one 4096 x 4096 frame."""
    i = np.arange(1 << 24, dtype=np.int64)
    bgr = np.stack([i & 255, (i >> 8) & 255, i >> 16], -1).astype(np.uint8).reshape(1, 4096, 4096, 3)
    got = ctx.gray(_dev(bgr)).cpu().numpy().reshape(-1)
    want = ((3735 * (i & 255) + 19235 * ((i >> 8) & 255) + 9798 * (i >> 16) + 16384) >> 15).astype(np.uint8)
    _report(got, want, "k_gray on all colours")


BLUR_SIZES = (1, 2, 3, 4, 5, 7, 8, 257)


def test_blur_every_ksize_and_shape(ctx):
    rs = np.random.RandomState(50)
    for H in BLUR_SIZES:
        for W in BLUR_SIZES:
            img = rs.randint(0, 256, (3, H, W)).astype(np.uint8)
            d = _dev(img)
            for k in (1, 3, 5, 7):
                _report(ctx.blur(d, k).cpu().numpy(), T.blur(img, k), f"k_blur {k} {H}x{W}")


@functools.lru_cache(maxsize=None)
def _threshold_inputs(block):
    """Tie-dense patches of this block, an image smaller than the block, and a noise image."""
    return [T.tie_image(2 * block + 3, 4 * block + 1, block, 60 + block)[None], T.BY_NAME["small_5x7"].data(),
            T.BY_NAME["noise_61x83"].data(), T.BY_NAME["one_row"].data(), T.BY_NAME["one_col"].data()]


@pytest.mark.parametrize("block", T.BLOCKS)
def test_adaptive_threshold_every_block_and_c(ctx, block):
    for img in _threshold_inputs(block):
        d = _dev(img)
        mean = T.adaptive_mean(img, block)
        for c in T.C_VALUES:
            for inv in (True, False):
                _report(ctx.adaptive_threshold(d, block, c, inv).cpu().numpy(), T.threshold_from_mean(img, mean, c, inv),
                        f"k_adaptive_threshold {img.shape} block {block} C={c} inv={inv}")


@pytest.mark.parametrize("case", [c for c in T.CASES if c.kind == "gray"], ids=lambda c: c.name)
def test_standalone_cases(ctx, case):
    imgs = case.data()
    d = _dev(imgs)
    for k in (3, 5, 7):
        _report(ctx.blur(d, k).cpu().numpy(), T.blur(imgs, k), f"{case.name} blur {k}")
    block = case.params.get("block", 11)
    for c, inv in ((2, True), (2, False), (2.5, False)):
        _report(ctx.adaptive_threshold(d, block, c, inv).cpu().numpy(), T.adaptive_threshold(imgs, block, c, inv),
                f"{case.name} threshold {block} C={c} inv={inv}")


@pytest.mark.parametrize("case", [c for c in T.CASES if c.kind == "frame"], ids=lambda c: c.name)
def test_fused_cases(ctx, case):
    frames = case.data()
    d = _dev(frames)
    _report(ctx.gray(d).cpu().numpy(), T.gray(frames), f"{case.name} gray")
    got = ctx.preprocess(d).cpu().numpy()
    for f in range(len(frames)):
        _report(got[f], T.preprocess(frames[f]), f"{case.name} frame {f}", frames[f])


# ---- N1 ---------------------------------------------------------------------------------------------------------------------------------
def test_preprocess_cells_on_order_sensitive_cells(ctx, golden_dir):
    """preprocess_cells and cnn_forward(glue=GLUE_RUNPY) on the cells whose CLAHE output has order-sensitive pixels: the threshold
    stage equals threshold_ref.adaptive_threshold(clahe(cell), 11, 2, BINARY) bit for bit, and the digits equal those of the CNN
    oracle fed with the restatement's cells."""
    cells, cl = T.order_sensitive_cells(o.clahe, T.tie_cells())
    assert len(cells) >= 8
    want = T.adaptive_threshold(cl, 11, 2, inv=False)
    d = _dev(cells)
    _report(ctx.preprocess_cells(d).cpu().numpy(), want, "preprocess_cells")
    g2 = np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz"))
    sd = {k: torch.from_numpy(g2[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS}
    ctx.load_state_dict(sd)
    logits, digits, _ = ctx.cnn_forward(d, want_digits=True, glue=Context.GLUE_RUNPY)
    el, ed, _ = cnn_oracle.predict(sd, o.cells_to_input(want)[:, None])
    assert np.abs(logits.cpu().numpy() - el.numpy()).max() <= 1e-4
    assert (digits.cpu().numpy() == ed.numpy()).all()
