"""CPU: the argument checks of runtime.Context.  The library sees only raw pointers, so every tensor argument is checked in Python
(runtime._dev_tensor) before any library call, and views are passed with their real row stride or made contiguous
(runtime._image_layout, runtime._frame_layout).  No GPU: tensors stay on the CPU and the expected device is cuda:0."""
import pytest
import torch

from sudoku_vision_amd import runtime as rt

CUDA0 = torch.device("cuda", 0)
CPU = torch.device("cpu")


def test_dev_tensor_rejects_kind_dtype_and_device():
    t = torch.zeros((2, 28, 28), dtype=torch.uint8)
    assert rt._dev_tensor(t, "t", torch.uint8, CPU, shape=(None, 28, 28)) is t
    with pytest.raises(TypeError, match="cuda:0"):
        rt._dev_tensor(t, "t", torch.uint8, CUDA0)
    with pytest.raises(TypeError, match="torch.Tensor"):
        rt._dev_tensor(t.numpy(), "t", torch.uint8, CPU)
    with pytest.raises(TypeError, match="dtype|torch.uint8"):
        rt._dev_tensor(t.float(), "t", torch.uint8, CPU)
    with pytest.raises(TypeError):
        rt._dev_tensor(t.to(torch.int8), "t", (torch.uint8, torch.int32), CPU)
    assert rt._dev_tensor(t.int(), "t", (torch.uint8, torch.int32), CPU) is not None
    assert rt._dev_tensor(t.double(), "t", None, CPU) is not None


def test_dev_tensor_rejects_shapes():
    t = torch.zeros((2, 32, 32), dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"\[\*,28,28\]"):
        rt._dev_tensor(t, "cells", torch.uint8, CPU, shape=(None, 28, 28))
    with pytest.raises(ValueError):
        rt._dev_tensor(t[0], "cells", torch.uint8, CPU, shape=(None, 28, 28))
    with pytest.raises(ValueError):
        rt._dev_tensor(t, "img", torch.uint8, CPU, ndim=(2, 4))
    assert rt._dev_tensor(t[:, 2:30, 2:30], "cells", torch.uint8, CPU, shape=(None, 28, 28)) is not None


def test_image_layout_passes_row_strides_of_dense_rows():
    frame = torch.arange(6 * 10 * 3, dtype=torch.int32).to(torch.uint8).reshape(6, 10, 3)
    v, pitch = rt._image_layout(frame[:, :5])                 # the left half: rows stay 30 bytes apart
    assert pitch == 30 and v.data_ptr() == frame.data_ptr()
    gray = frame[..., 0].contiguous()
    v, pitch = rt._image_layout(gray[1:5, 3:9])               # a gray crop: read in place
    assert pitch == 10 and v.data_ptr() == gray[1:5, 3:9].data_ptr()
    v, pitch = rt._image_layout(gray.t())                     # columns are not dense: copied
    assert v.is_contiguous() and pitch == 6 and torch.equal(v, gray.t())
    v, pitch = rt._image_layout(frame[:, :, :2])              # two of three channels: copied
    assert v.is_contiguous() and pitch == 20
    v, pitch = rt._image_layout(frame[:, ::2])                # every other column: copied
    assert v.is_contiguous() and pitch == 15
    v, pitch = rt._image_layout(gray[2:3])                    # one row: its own width
    assert pitch == 10
    v, pitch = rt._image_layout(gray)
    assert pitch == 10 and v is gray


def test_frame_layout_checks_device_dtype_and_shape():
    f = torch.zeros((2, 4, 6, 3), dtype=torch.uint8)
    with pytest.raises(TypeError):
        rt._frame_layout(f, CUDA0)
    with pytest.raises(ValueError):
        rt._frame_layout(f[..., :1], CPU)
    with pytest.raises(TypeError):
        rt._frame_layout(f.float(), CPU)
    v, pitch, stride = rt._frame_layout(f[:, :, :3], CPU)
    assert (pitch, stride) == (18, 72) and v.data_ptr() == f.data_ptr()


class _NoLibrary:
    """Stands in for the native library: any call is a failure (the checks must come first)."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} reached with a bad argument")


@pytest.fixture
def ctx():
    c = object.__new__(rt.Context)          # no GPU here: skip __init__'s device and library set-up
    c.device, c._lib, c._h = CUDA0, _NoLibrary(), None
    return c


def _u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


def test_every_method_rejects_host_tensors_before_the_library(ctx):
    frames, gray, cells = _u8(2, 20, 24, 3), _u8(2, 20, 24), _u8(5, 28, 28)
    minv = torch.eye(3, dtype=torch.float64)[None].repeat(2, 1, 1)
    calls = [
        lambda: ctx.gray(frames), lambda: ctx.blur(gray, 5), lambda: ctx.adaptive_threshold(gray, 11, 2),
        lambda: ctx.preprocess(frames), lambda: ctx.preprocess_and_warp_cells(frames, minv), lambda: ctx.preprocess_bits(_u8(2, 20, 32, 3)),
        lambda: ctx.despeckle(gray), lambda: ctx.despeckle_bits(torch.zeros((2, 20, 1), dtype=torch.int32)),
        lambda: ctx.pack_sparse_bits(torch.zeros((2, 20, 1), dtype=torch.int32), _u8(2, 64)),
        lambda: ctx.warp_perspective(frames[0], minv[0], 64), lambda: ctx.warp_perspective(gray[0], minv[0], 64),
        lambda: ctx.extract_cells(_u8(45, 45), 28, 0, 0), lambda: ctx.warp_cells(frames, minv),
        lambda: ctx.resize_linear(gray[0], (28, 28)), lambda: ctx.cell_ink_ratio(cells), lambda: ctx.preprocess_cells(cells),
        lambda: ctx.cnn_forward(cells), lambda: ctx.cnn_forward(torch.zeros((5, 1, 28, 28))), lambda: ctx.softmax_topk(torch.zeros((5, 10))),
        lambda: ctx.frames_to_digits(frames, minv), lambda: ctx.frame_quality_stats(frames), lambda: ctx.frame_quality_stats(gray),
        lambda: ctx.grid_line_coverage(gray, minv), lambda: ctx.grid_line_coverage(torch.zeros((2, 20, 1), dtype=torch.int32), minv),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(TypeError, match="cuda:0"):
            call()


def test_minv_on_the_host_is_rejected(ctx, monkeypatch):
    """A host minv with device frames: the minv check fires (the frames pass a stubbed layout check)."""
    monkeypatch.setattr(rt, "_frame_layout", lambda f, d=None: (f, 72, 1440))
    with pytest.raises(TypeError, match="minv_dev"):
        ctx.warp_cells(_u8(2, 20, 24, 3), torch.eye(3, dtype=torch.float64)[None].repeat(2, 1, 1))
    with pytest.raises(TypeError, match="minv_dev"):
        ctx.frames_to_digits(_u8(2, 20, 24, 3), torch.eye(3, dtype=torch.float64)[None].repeat(2, 1, 1))


def test_cell_shapes_are_checked_first(ctx, monkeypatch):
    """preprocess_cells and the u8 cnn_forward take 28x28 cells only: [B,32,32] (or its uncropped view) is a ValueError, not a
    launch over the wrong pixels.  The device check is stubbed so that the shape check is what fails."""
    real = rt._dev_tensor

    def on_device(t, name, dtype, device, shape=None, ndim=None):
        return real(t, name, dtype, CPU, shape, ndim)

    monkeypatch.setattr(rt, "_dev_tensor", on_device)
    big = _u8(4, 32, 32)
    for call in (lambda c: ctx.preprocess_cells(c), lambda c: ctx.cnn_forward(c)):
        with pytest.raises(ValueError, match="28"):
            call(big)
    with pytest.raises(ValueError):
        ctx.cnn_forward(torch.zeros((4, 3, 28, 28)))
    with pytest.raises(ValueError):
        ctx.warp_perspective(_u8(20, 24, 2), torch.eye(3, dtype=torch.float64), 64)
    with pytest.raises(ValueError):
        ctx.warp_perspective(_u8(20, 24, 3), torch.eye(3, dtype=torch.float64)[None].repeat(2, 1, 1), 64)
    with pytest.raises(TypeError):
        ctx.warp_perspective(_u8(20, 24, 3), torch.eye(3, dtype=torch.float32), 64)
    with pytest.raises(TypeError):
        ctx.resize_linear(torch.zeros((20, 24), dtype=torch.int16), (28, 28))
