"""CPU: the argument checks of runtime.Context.  The library sees only raw pointers, so every tensor argument is checked in Python
(runtime._dev_tensor) before any library call, and views are passed with their real row stride or made contiguous
(runtime._image_layout, runtime._frame_layout).  No GPU: tensors stay on the CPU and the expected device is cuda:0.
Also the host-side helpers the drop-ins share: the array conversion (runtime._to_dev / _back) and the state-dict blob (runtime._state_blob)."""
import types

import numpy as np
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


def test_plane_and_frame_layout_are_one_rule():
    """Padded rows and frame gaps pass through with their strides; one frame has stride pitch * H; anything else is copied."""
    g = torch.arange(3 * 6 * 10, dtype=torch.int32).to(torch.uint8).reshape(3, 6, 10)
    v, pitch, stride = rt._plane_layout(g[:, 1:5, 2:9], CPU)             # cropped rows and columns: read in place
    assert (pitch, stride) == (10, 60) and v.data_ptr() == g[:, 1:5, 2:9].data_ptr()
    v, pitch, stride = rt._plane_layout(g[::2], CPU)                     # every other frame: a gap
    assert (pitch, stride) == (10, 120) and v.data_ptr() == g.data_ptr()
    v, pitch, stride = rt._plane_layout(g[1:2, :, :7], CPU)              # one frame
    assert (pitch, stride) == (10, 60)
    v, pitch, stride = rt._plane_layout(g[:, :, ::2], CPU)               # every other column: copied
    assert v.is_contiguous() and (pitch, stride) == (5, 30) and torch.equal(v, g[:, :, ::2])
    v, pitch, stride = rt._plane_layout(g.permute(0, 2, 1), CPU)            # transposed: copied
    assert v.is_contiguous() and (pitch, stride) == (6, 60)
    f = torch.zeros((2, 4, 6, 3), dtype=torch.uint8)
    v, pitch, stride = rt._frame_layout(f[:, :, ::2], CPU)                  # every other pixel: copied
    assert v.is_contiguous() and (pitch, stride) == (9, 36)
    v, pitch, stride = rt._frame_layout(torch.zeros((2, 4, 6, 4), dtype=torch.uint8)[..., :3], CPU)   # BGRA's first three: copied
    assert v.is_contiguous() and (pitch, stride) == (18, 72)
    with pytest.raises(TypeError, match="cuda:0"):
        rt._plane_layout(g, CUDA0)
    with pytest.raises(ValueError):
        rt._plane_layout(g[0], CPU)
    with pytest.raises(TypeError):
        rt._plane_layout(g.float(), CPU)


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
        lambda: ctx.cnn3_forward(cells), lambda: ctx.cnn3_forward(torch.zeros((5, 1, 28, 28))), lambda: ctx.frames_to_digits_v3(frames, minv),
        lambda: ctx.preprocess_mm(frames), lambda: ctx.morphology(gray, ctx.MORPH_CLOSE, ctx.SHAPE_RECT, 3), lambda: ctx.box_mean(gray, 5),
        lambda: ctx.gaussian_blur21(gray), lambda: ctx.divide_normalize(gray, gray), lambda: ctx.clahe(gray),
        lambda: ctx.threshold_sauvola(gray), lambda: ctx.threshold_count(gray, 128), lambda: ctx.shadow_mask(gray, gray),
        lambda: ctx.count_nonzero(gray), lambda: ctx.copy_to_pinned(gray, torch.zeros_like(gray)),
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


def test_both_images_of_a_two_image_method_are_checked(ctx, monkeypatch):
    """divide_normalize and shadow_mask read a second image.  With both on the host the first argument is the one reported; with the first
    passing a stubbed layout check (which records that it was reached) the second is."""
    host = _u8(2, 20, 24)
    with pytest.raises(TypeError, match="gray must be on cuda:0"):
        ctx.divide_normalize(host, host)
    with pytest.raises(TypeError, match="gray must be on cuda:0"):
        ctx.shadow_mask(host, host)
    reached = []

    def first_passes(x, device, name="gray"):
        reached.append(name)
        return x, 24, 480

    monkeypatch.setattr(rt, "_plane_layout", first_passes)
    with pytest.raises(TypeError, match="background must be on cuda:0"):
        ctx.divide_normalize(host, host)
    with pytest.raises(TypeError, match="local_mean must be on cuda:0"):
        ctx.shadow_mask(host, host)
    assert reached == ["gray", "gray"]


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


@pytest.mark.gpu
def test_cross_check_selections_are_unknown_to_the_product():
    """SV_CNN_X_WINOGRAD (102) and SV_CNN_X_WSPLIT (103) name kernels of the test-only library: a product context rejects them and keeps
    its selection, a context of libsudokuvision_xcheck.so takes them.  Needs a context (so a device) but launches nothing."""
    import sudoku_vision_amd as sva
    product, xc = sva.Context(), sva.Context(library=sva._native.lib_xcheck())
    try:
        for which, algo in ((rt.Context.CNN_X_WINOGRAD, 2), (rt.Context.CNN_X_WSPLIT, 3)):
            with pytest.raises(sva._native.NativeError, match=rf"SV_ERR_BAD_ARG: sv_ctx_set_cnn_kernels: unknown selection {which}$"):
                product.set_cnn_kernels(which)
            assert product.conv_kernel_info()["algo"] in (0, 4)      # still SV_CNN_AUTO: f32-MFMA or f16 pairs
            xc.set_cnn_kernels(which)
            assert xc.conv_kernel_info()["algo"] == algo
    finally:
        product.close()
        xc.close()


# ---- the drop-ins' array conversion ------------------------------------------------------------------------------------
@pytest.fixture
def cpu_ctx():
    """Stands in for a Context in _to_dev, which reads its device only: uploads stay on the CPU."""
    return types.SimpleNamespace(device=CPU)


def test_to_dev_takes_numpy_uint8_and_gives_numpy_back(cpu_ctx):
    a = np.arange(24, dtype=np.uint8).reshape(4, 6)
    t, was_tensor = rt._to_dev(a, cpu_ctx)
    assert isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.device == CPU and was_tensor is False
    assert tuple(t.shape) == (4, 6) and (t.numpy() == a).all()
    back = rt._back(t, was_tensor)
    assert isinstance(back, np.ndarray) and back.dtype == np.uint8 and (back == a).all()
    assert rt._back(t, True) is t                                      # a tensor argument gets the tensor itself back
    t, _ = rt._to_dev(a[:, ::2], cpu_ctx)                              # a view: its values, dense
    assert (t.numpy() == a[:, ::2]).all()


def test_to_dev_aliases_a_contiguous_numpy_input(cpu_ctx):
    a = np.zeros((4, 6), np.uint8)
    t, _ = rt._to_dev(a, cpu_ctx)
    a[2, 3] = 77
    assert int(t[2, 3]) == 77 and t.data_ptr() == a.ctypes.data


@pytest.mark.parametrize("bad", [np.zeros((4, 6), np.float32), np.zeros((4, 6), np.int8), np.zeros((4, 6), np.uint16), [[0.5, 1.5]]])
def test_to_dev_rejects_arrays_that_are_not_uint8(cpu_ctx, bad):
    with pytest.raises(TypeError, match="uint8"):
        rt._to_dev(bad, cpu_ctx)


def test_to_dev_rejects_cpu_and_float_tensors(cpu_ctx):
    with pytest.raises(TypeError, match="CUDA"):
        rt._to_dev(torch.zeros((4, 6), dtype=torch.uint8), cpu_ctx)    # a CPU tensor, even where the context's device is the CPU
    with pytest.raises(TypeError, match="uint8"):
        rt._to_dev(torch.zeros((4, 6)), cpu_ctx)
    with pytest.raises(TypeError):
        rt._to_dev(torch.zeros((4, 6), dtype=torch.uint8), types.SimpleNamespace(device=CUDA0))


# ---- state_dict -> blob ------------------------------------------------------------------------------------------------
def test_state_blob_of_the_v1_model_is_the_tensors_in_layout_order():
    import cnn_oracle
    sd = cnn_oracle.random_state_dict(1234)
    blob = rt._state_blob(sd, rt._V1_LAYOUT, "DigitCNN")
    assert blob.dtype == np.float32 and blob.shape == (421642,)
    assert [k for k, _ in rt._V1_LAYOUT] == ["conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
    at = 0
    for k, shape in rt._V1_LAYOUT:
        v = np.asarray(sd[k].detach().cpu().numpy() if isinstance(sd[k], torch.Tensor) else sd[k], np.float32)
        assert tuple(v.shape) == shape
        assert (blob[at:at + v.size] == v.reshape(-1)).all(), k
        at += v.size
    assert at == 421642
    as_arrays = {k: np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, np.float64) for k, v in sd.items()}
    assert (rt._state_blob(as_arrays, rt._V1_LAYOUT, "DigitCNN") == blob).all()      # arrays of another dtype: converted to f32


def test_state_blob_names_the_key_of_a_wrong_shape():
    import cnn_oracle
    sd = dict(cnn_oracle.random_state_dict(1))
    sd["fc1.bias"] = torch.zeros(127)
    with pytest.raises(ValueError, match="fc1.bias"):
        rt._state_blob(sd, rt._V1_LAYOUT, "DigitCNN")
    sd["fc1.bias"] = torch.zeros(128, 1)
    with pytest.raises(ValueError, match="fc1.bias"):
        rt._state_blob(sd, rt._V1_LAYOUT, "DigitCNN")


@pytest.mark.parametrize("use_se", [True, False])
def test_state_blob_misses_a_v3_key(use_se):
    layout = rt.v3_layout(use_se)
    sd = {k: np.zeros(shape, np.float32) for k, shape in layout}
    assert rt._state_blob(sd, layout, "DigitCNNv3").size == sum(int(np.prod(shape)) for _, shape in layout)
    for gone in ("temperature", "layer2.shortcut.1.running_var", "fc.bias"):
        with pytest.raises(KeyError, match=gone.replace(".", r"\.")):
            rt._state_blob({k: v for k, v in sd.items() if k != gone}, layout, "DigitCNNv3")
    with pytest.raises(KeyError):
        rt._state_blob({}, rt._V1_LAYOUT, "DigitCNN")
