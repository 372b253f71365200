"""Device context and the device-resident entry point of the hot path.

One `Context` per (process, GPU): it owns the packed CNN weights and the scratch the kernels use.
Tensors are PyTorch-ROCm tensors; the library sees raw pointers and the current HIP stream.
"""
import ctypes as C
import threading

import numpy as np
import torch

from . import _native

# (key, shape) of a DigitCNN state_dict (ml/model.py) in the order of the blob sv_load_weights_f32 takes
_V1_LAYOUT = (("conv1.weight", (32, 1, 3, 3)), ("conv1.bias", (32,)), ("conv2.weight", (64, 32, 3, 3)), ("conv2.bias", (64,)),
              ("fc1.weight", (128, 3136)), ("fc1.bias", (128,)), ("fc2.weight", (10, 128)), ("fc2.bias", (10,)))


# DigitCNNv3 (ml/model_v3.py): (in, out, stride) of layer1..5
_V3_BLOCKS = ((32, 32, 1), (32, 64, 2), (64, 64, 1), (64, 128, 2), (128, 128, 1))


def v3_layout(use_se=True):
    """(key, shape) of every float entry of a DigitCNNv3 state_dict, in key order: the blob sv_load_weights_v3_f32 takes.  The int64
    num_batches_tracked entries are not part of it."""
    def bn(prefix, c):
        return [(f"{prefix}.{n}", (c,)) for n in ("weight", "bias", "running_mean", "running_var")]
    out = [("temperature", (1,)), ("stem.0.weight", (32, 1, 3, 3))] + bn("stem.1", 32)
    for i, (cin, c, stride) in enumerate(_V3_BLOCKS, 1):
        L = f"layer{i}"
        out += [(f"{L}.conv1.weight", (c, cin, 3, 3))] + bn(f"{L}.bn1", c) + [(f"{L}.conv2.weight", (c, c, 3, 3))] + bn(f"{L}.bn2", c)
        if use_se:
            out += [(f"{L}.se.excite.0.weight", (c // 4, c)), (f"{L}.se.excite.2.weight", (c, c // 4))]
        if stride != 1 or cin != c:
            out += [(f"{L}.shortcut.0.weight", (c, cin, 1, 1))] + bn(f"{L}.shortcut.1", c)
    return out + [("fc.weight", (10, 128)), ("fc.bias", (10,))]


def light_layout():
    """(key, shape) of every float entry of a DigitCNNv3Light state_dict (ml/model_v3.py), in key order: the blob
    sv_load_weights_v3_light_f32 takes.  The int64 num_batches_tracked entries are not part of it."""
    out = [("temperature", (1,))]
    for i, (cin, c) in zip((0, 4, 8), ((1, 24), (24, 48), (48, 96))):
        out += [(f"features.{i}.weight", (c, cin, 3, 3))] + [(f"features.{i + 1}.{n}", (c,)) for n in ("weight", "bias", "running_mean", "running_var")]
    return out + [("fc.weight", (10, 96)), ("fc.bias", (10,))]


def empty_layout():
    """(key, shape) of an EmptyClassifier state_dict (ml/model_v3.py), in key order: the blob sv_load_weights_empty_f32 takes."""
    return [("features.0.weight", (16, 1, 3, 3)), ("features.0.bias", (16,)), ("features.3.weight", (32, 16, 3, 3)), ("features.3.bias", (32,)),
            ("classifier.1.weight", (32, 1568)), ("classifier.1.bias", (32,)), ("classifier.4.weight", (1, 32)), ("classifier.4.bias", (1,))]


def _state_blob(sd, layout, model, strict=False):
    """sd: a state_dict of `model` -- tensors or arrays, any device -> its `layout` entries ((key, shape) pairs) as one float32 host
    array in that order.  KeyError for a missing key, ValueError for a wrong shape; entries outside the layout are not looked at, or with
    `strict` are a ValueError unless they are num_batches_tracked counters."""
    if strict:
        known = dict(layout)
        extra = [k for k in sd if not k.endswith("num_batches_tracked") and k not in known]
        if extra:
            raise ValueError(f"not {model} keys: {extra[:4]}")
    parts = []
    for k, shape in layout:
        if k not in sd:
            raise KeyError(f"{model} state_dict lacks {k}")
        v = sd[k]
        v = v.detach().to("cpu", torch.float32).numpy() if isinstance(v, torch.Tensor) else np.asarray(v, np.float32)
        if tuple(v.shape) != shape:
            raise ValueError(f"{k}: shape {tuple(v.shape)} != {shape}")
        parts.append(np.ascontiguousarray(v).reshape(-1))
    return np.concatenate(parts)


def _require_gpu():
    if not torch.cuda.is_available():
        raise _native.NativeError("no ROCm GPU visible: the sudoku-vision hot path runs on MI355X only (no CPU fallback)")


def _stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _opt_ptr(t):
    """_ptr of an output the caller may not want: NULL for None."""
    return None if t is None else _ptr(t)


def _dev_tensor(t, name, dtype, device, shape=None, ndim=None):
    """Check a tensor argument before anything reaches the library, which sees only its data pointer: a torch.Tensor of `dtype`
    (a dtype, a tuple of them, or None for any) on `device`, of `shape` (None entries match any size) or with `ndim` dimensions
    (an int or a tuple of them).  TypeError for the kind, dtype or device; ValueError for the shape.  Returns t."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if dtype is not None and t.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,)):
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if t.device != torch.device(device):
        raise TypeError(f"{name} must be on {device}, got {t.device}")
    if shape is not None:
        if t.dim() != len(shape) or any(want is not None and got != want for got, want in zip(t.shape, shape)):
            raise ValueError(f"{name} must have shape [{','.join('*' if v is None else str(v) for v in shape)}], got {list(t.shape)}")
    elif ndim is not None and t.dim() not in (ndim if isinstance(ndim, tuple) else (ndim,)):
        raise ValueError(f"{name} must have {ndim} dimensions, got {list(t.shape)}")
    return t


def _image_layout(img):
    """img u8 [H,W] or [H,W,C]: (tensor, row pitch in bytes).  A view whose rows are dense (cropped columns, padded rows) is passed
    through with its own row stride; anything else is made contiguous first."""
    H, W = img.shape[0], img.shape[1]
    ch = 1 if img.dim() == 2 else img.shape[2]
    st = img.stride()
    dense_rows = st[1] == ch and (img.dim() == 2 or st[2] == 1 or ch == 1)
    if H == 1 and dense_rows:
        return img, W * ch
    if not (dense_rows and st[0] >= W * ch):
        img = img.contiguous()
        st = img.stride()
    return img, st[0]


def _batch_layout(x, device, name, ch):
    """x u8 [n,H,W] (ch = 1) or [n,H,W,ch] on device: (tensor, row pitch, frame stride) in bytes.  Row padding, gaps between frames and any
    base alignment are passed through to the library (camera buffers are rarely dense); anything else is made contiguous first."""
    _dev_tensor(x, name, torch.uint8, device, shape=(None, None, None, ch) if ch > 1 else (None, None, None))
    n, H, row = x.shape[0], x.shape[1], x.shape[2] * ch                # a row of W pixels is W * ch dense bytes
    st = x.stride()
    # st[2] is the pixel stride and st[-1] the channel stride; for planes both name the pixel stride
    if not (st[-1] == 1 and st[2] == ch and st[1] >= row and (n == 1 or st[0] >= st[1] * (H - 1) + row)):
        x = x.contiguous()
        st = x.stride()
    return x, st[1], (st[0] if n > 1 else st[1] * H)


def _frame_layout(frames, device):
    """frames u8 [n,H,W,3] on device: _batch_layout of BGR frames."""
    return _batch_layout(frames, device, "frames", 3)


def _plane_layout(x, device, name="gray"):
    """x u8 [n,H,W] on device: _batch_layout of gray planes."""
    return _batch_layout(x, device, name, 1)


def _to_dev(a, ctx):
    """An image argument of a drop-in (cv/*.py) -> (u8 tensor on ctx's device, was_tensor).  A numpy uint8 array is uploaded; a uint8 CUDA
    tensor is passed as it is, views included: the Context methods deal with layout.  Anything else is a TypeError."""
    if isinstance(a, torch.Tensor):
        if a.dtype != torch.uint8 or not a.is_cuda:
            raise TypeError("expected a uint8 CUDA tensor or a numpy uint8 array")
        return a, True
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise TypeError(f"expected uint8 image, got {a.dtype}")
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device), False


def _back(t, was_tensor):
    """A drop-in's result in the kind its argument had: the tensor itself, or a numpy array on the host."""
    return t if was_tensor else t.cpu().numpy()


def _model_context(x, training, name, eval_note):
    """The preamble of the drop-in models' forward (ml/*.py): inference only, CUDA only, x [batch,1,28,28] -> the context of x's device."""
    if training:
        raise NotImplementedError(f"{name} (MI355X): inference only -- call .eval() ({eval_note} in eval mode)")
    if not x.is_cuda:
        raise RuntimeError(f"{name} (MI355X): input must be a CUDA tensor; there is no CPU fallback")
    if x.dim() != 4 or tuple(x.shape[1:]) != (1, 28, 28):
        raise ValueError(f"expected input of shape (batch, 1, 28, 28), got {tuple(x.shape)}")
    return default_context(x.device)


class Context:
    def __init__(self, device=None, library=None):
        """library: a handle from _native (default: the product library).  Tests pass _native.lib_xcheck() to run the cross-check kernels of
        the test-only build through the same methods."""
        _require_gpu()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else torch.device(device).index or 0)
        self._lib = library or _native.lib()
        self._h = C.c_void_p()
        self._check(self._lib.sv_ctx_create(self.device.index, C.byref(self._h)), "sv_ctx_create")
        self._weights_key = None
        self._weights_v3_key = None
        self._weights_light_key = None
        self._weights_empty_key = None

    def _check(self, rc, what):
        _native.check(rc, what, self._lib)

    def _out(self, t, shape, dtype, name):
        """An output tensor: a new one, or the caller's `t`.  The kernels write shape-many elements through its raw pointer, so `t` has to
        be exactly that."""
        if t is None:
            return torch.empty(tuple(shape), dtype=dtype, device=self.device)
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous() or t.device != self.device:
            raise TypeError(f"{name} must be a contiguous {dtype} tensor of shape {list(shape)} on {self.device}")
        return t

    def _minv(self, minv_dev, n):
        """minv_dev: n destination -> source maps, float64 [n,3,3] (or any shape of 9n elements) on this device."""
        _dev_tensor(minv_dev, "minv_dev", torch.float64, self.device)
        if minv_dev.numel() != 9 * n:
            raise ValueError(f"minv_dev must hold {n} 3x3 matrices, got shape {list(minv_dev.shape)}")
        return minv_dev.contiguous()

    def close(self):
        if self._h:
            self._lib.sv_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights ------------------------------------------------------------------------------
    def load_state_dict(self, sd, key=None):
        """sd: DigitCNN state_dict (ml/model.py) -- tensors or arrays, any device."""
        blob = _state_blob(sd, _V1_LAYOUT, "DigitCNN")
        self._check(self._lib.sv_load_weights_f32(self._h, blob.ctypes.data_as(C.c_void_p)), "sv_load_weights_f32")
        self._weights_key = key

    def load_state_dict_v3(self, sd, use_se=None, key=None):
        """sd: DigitCNNv3 state_dict (ml/model_v3.py) -- tensors or arrays, any device; num_batches_tracked entries are ignored.
        use_se: None = inferred from the keys.  Independent of load_state_dict: one context holds both models."""
        has_se = any(".se.excite." in k for k in sd)
        if use_se is None:
            use_se = has_se
        elif bool(use_se) != has_se:
            raise ValueError(f"use_se={use_se} but the state_dict {'has' if has_se else 'has no'} se.excite weights")
        blob = _state_blob(sd, v3_layout(bool(use_se)), "DigitCNNv3", strict=True)
        self._check(self._lib.sv_load_weights_v3_f32(self._h, blob.ctypes.data_as(C.c_void_p), blob.size, int(bool(use_se))), "sv_load_weights_v3_f32")
        self._weights_v3_key = key

    def load_state_dict_v3_light(self, sd, key=None):
        """sd: DigitCNNv3Light state_dict (ml/model_v3.py) -- tensors or arrays, any device; num_batches_tracked entries are ignored.
        A weight slot of its own: the other models' weights stay as they are."""
        blob = _state_blob(sd, light_layout(), "DigitCNNv3Light", strict=True)
        self._check(self._lib.sv_load_weights_v3_light_f32(self._h, blob.ctypes.data_as(C.c_void_p), blob.size), "sv_load_weights_v3_light_f32")
        self._weights_light_key = key

    def load_state_dict_empty(self, sd, key=None):
        """sd: EmptyClassifier state_dict (ml/model_v3.py) -- tensors or arrays, any device.  A weight slot of its own."""
        blob = _state_blob(sd, empty_layout(), "EmptyClassifier", strict=True)
        self._check(self._lib.sv_load_weights_empty_f32(self._h, blob.ctypes.data_as(C.c_void_p), blob.size), "sv_load_weights_empty_f32")
        self._weights_empty_key = key

    PREC_F32, PREC_BF16 = 0, 1

    def set_precision(self, precision):
        """PREC_F32 (default, logits within 1e-4 of the reference model) or PREC_BF16 (bf16 MFMA, digit-index parity)."""
        self._check(self._lib.sv_ctx_set_precision(self._h, int(precision)), "sv_ctx_set_precision")

    CNN_AUTO, CNN_F16PAIR, CNN_F32MFMA = 0, 1, 2
    CNN_X_WINOGRAD, CNN_X_WSPLIT = 102, 103          # cross-check selections of the test-only library (include/sudoku_vision_xcheck.h)

    def set_cnn_kernels(self, which):
        """CNN_AUTO (default: the f16-pair kernels whenever the weights / inputs are inside their range, else the f32-MFMA kernels),
        CNN_F16PAIR or CNN_F32MFMA (sv_ctx_set_cnn_kernels)."""
        self._check(self._lib.sv_ctx_set_cnn_kernels(self._h, int(which)), "sv_ctx_set_cnn_kernels")

    def reserve(self, max_cells):
        self._check(self._lib.sv_ctx_reserve(self._h, int(max_cells)), "sv_ctx_reserve")

    # ---- per-kernel timing (hipEvents on the launch stream, inside the library) -------------------
    KERNELS = ("k_preprocess", "k_warp_cells", "k_conv_features", "k_fc_head", "k_preprocess_warp_fused", "k_harris", "k_warp_affine")

    def timing_begin(self):
        self._check(self._lib.sv_timing_begin(self._h), "sv_timing_begin")

    def timing_end(self):
        """-> {kernel name: (total ms, launches)}; waits for the recorded events."""
        ms = (C.c_double * len(self.KERNELS))()
        cnt = (C.c_long * len(self.KERNELS))()
        self._check(self._lib.sv_timing_end(self._h, ms, cnt, len(self.KERNELS)), "sv_timing_end")
        return {k: (ms[i], cnt[i]) for i, k in enumerate(self.KERNELS)}

    CONV_ALGO_NAMES = {0: "k_conv_features_pc + k_fc_head (direct implicit GEMM, f32 MFMA)",
                       2: "k_conv_features_wstream (Winograd F(2x2,3x3), f32 MFMA; cross-check build)",
                       3: "k_conv_features_wsplit (Winograd, bf16 MFMA with 3-way operand split; cross-check build)",
                       4: "k_conv_features_h2 + k_fc_head_h2p (f16 hi/lo operand pairs, f16 MFMA, f32 accumulation)"}

    def conv_kernel_info(self):
        """Which conv/fc kernels this process launches and the matrix instructions they issue per cell (sv_conv_kernel_info)."""
        v = [C.c_int() for _ in range(5)]
        self._check(self._lib.sv_conv_kernel_info(self._h, *[C.byref(x) for x in v]), "sv_conv_kernel_info")
        a = v[0].value
        return {"algo": a, "name": self.CONV_ALGO_NAMES.get(a, str(a)), "mfma_conv2": v[1].value, "mfma_conv1": v[2].value,
                "mfma_f16_conv": v[3].value, "mfma_f16_fc": v[4].value}

    # ---- K1 -----------------------------------------------------------------------------------
    def gray(self, bgr):
        bgr, pitch, fstride = _frame_layout(bgr, self.device)
        n, H, W = bgr.shape[0], bgr.shape[1], bgr.shape[2]
        out = torch.empty((n, H, W), dtype=torch.uint8, device=self.device)
        self._check(self._lib.sv_gray_u8(self._h, _ptr(bgr), n, H, W, pitch, fstride, _ptr(out), _stream_ptr()), "sv_gray_u8")
        return out

    def blur(self, gray, ksize):
        gray = _dev_tensor(gray, "gray", torch.uint8, self.device, ndim=3).contiguous()
        n, H, W = gray.shape
        out = torch.empty_like(gray)
        self._check(self._lib.sv_blur_u8(self._h, _ptr(gray), n, H, W, int(ksize), _ptr(out), _stream_ptr()), "sv_blur_u8")
        return out

    def adaptive_threshold(self, gray, block_size, c, inv=True):
        gray = _dev_tensor(gray, "gray", torch.uint8, self.device, ndim=3).contiguous()
        n, H, W = gray.shape
        out = torch.empty_like(gray)
        self._check(self._lib.sv_adaptive_threshold_u8(self._h, _ptr(gray), n, H, W, int(block_size), float(c), int(bool(inv)),
                                                             _ptr(out), _stream_ptr()), "sv_adaptive_threshold_u8")
        return out

    def preprocess(self, frames, out=None):
        """frames u8 [n,H,W,3] on device (rows may be padded, frames may have gaps) -> binary u8 [n,H,W]
        (preprocess_for_grid_detection).  out: optional contiguous u8 [n,H,W] tensor to write into."""
        frames, pitch, fstride = _frame_layout(frames, self.device)
        n, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
        out = self._out(out, (n, H, W), torch.uint8, "out")
        self._check(self._lib.sv_preprocess_u8(self._h, _ptr(frames), n, H, W, pitch, fstride, _ptr(out), _stream_ptr()), "sv_preprocess_u8")
        return out

    def preprocess_and_warp_cells(self, frames, minv_dev, binary=None, cells=None):
        """K1 and K2 of the same frames in one launch (sv_preprocess_warp_cells_u8; BASELINE configs[4]'s fused threshold/warp for callers
        that know the corners beforehand) -> (binary u8 [n,H,W], cells u8 [n,81,28,28])."""
        frames, pitch, fstride = _frame_layout(frames, self.device)
        n, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
        minv_dev = self._minv(minv_dev, n)
        binary = self._out(binary, (n, H, W), torch.uint8, "binary")
        cells = self._out(cells, (n, 81, 28, 28), torch.uint8, "cells")
        self._check(self._lib.sv_preprocess_warp_cells_u8(self._h, _ptr(frames), n, H, W, pitch, fstride, _ptr(binary), _ptr(minv_dev), _ptr(cells),
                                                                _stream_ptr()), "sv_preprocess_warp_cells_u8")
        return binary, cells

    def preprocess_mm(self, frames, want_mean=False):
        """preprocess() through the matrix-pipe formulation of K1 (sv_preprocess_mm_u8): the same binary, an independent implementation.
        Only on a Context of the test-only library (Context(library=_native.lib_xcheck())).
        want_mean: also return the kernel's approximate local mean per pixel (f32 [n,H,W])."""
        frames, pitch, fstride = _frame_layout(frames, self.device)
        n, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
        out = torch.empty((n, H, W), dtype=torch.uint8, device=self.device)
        mean = torch.zeros((n, H, W), dtype=torch.float32, device=self.device) if want_mean else None
        self._check(self._lib.sv_preprocess_mm_u8(self._h, _ptr(frames), n, H, W, pitch, fstride, _ptr(out), _opt_ptr(mean),
                                                        _stream_ptr()), "sv_preprocess_mm_u8")
        return (out, mean) if want_mean else out

    def preprocess_stats(self):
        """(pixels decided by the exact evaluation in preprocess_mm launches since the last call, 0); the first call switches the counter on.
        Synchronises."""
        a, c = C.c_uint(), C.c_ulong()
        self._check(self._lib.sv_preprocess_stats(self._h, C.byref(a), C.byref(c)), "sv_preprocess_stats")
        return a.value, c.value

    def preprocess_bits(self, frames, out=None):
        """K1 with the binary as 1 bit per pixel: frames u8 [n,H,W,3] -> int32 [n,H,W//32] (LSB = leftmost pixel).  Needs W % 32 == 0 and
        4-byte aligned rows (NativeError SV_ERR_UNSUPPORTED otherwise: use preprocess + despeckle(packed=...))."""
        frames, pitch, fstride = _frame_layout(frames, self.device)
        n, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
        if W % 32:
            raise ValueError("preprocess_bits needs W % 32 == 0")
        out = self._out(out, (n, H, W // 32), torch.int32, "out")
        self._check(self._lib.sv_preprocess_bits_u8(self._h, _ptr(frames), n, H, W, pitch, fstride, _ptr(out), _stream_ptr()), "sv_preprocess_bits_u8")
        return out

    def despeckle_bits(self, bits):
        """despeckle on a bit image int32 [n,H,W//32], in place."""
        self._out(_dev_tensor(bits, "bits", torch.int32, self.device, ndim=3), bits.shape, torch.int32, "bits")
        n, H, wpr = bits.shape
        self._check(self._lib.sv_despeckle_bits(self._h, _ptr(bits), n, H, wpr * 32, _stream_ptr()), "sv_despeckle_bits")
        return bits

    def despeckle(self, binary, out=None, packed=None):
        """binary u8 [n,H,W] in {0,255} -> the same with the components that lie strictly inside a 64x64 tile erased (all of them,
        except in a tile whose flood fill hits its iteration cap: that tile is left as it is for that pass; sv_despeckle_u8 in the header)
        (find_grid_contour-equivalent; used only to make the host corner search cheaper).  packed: optional int32 [n,H,W//32]
        tensor receiving the result as 1 bit per pixel (then `out` is scratch)."""
        binary = _dev_tensor(binary, "binary", torch.uint8, self.device, ndim=3).contiguous()
        n, H, W = binary.shape
        out = self._out(out, (n, H, W), torch.uint8, "out")
        if packed is not None:
            self._out(packed, (n, H, W // 32), torch.int32, "packed")
        self._check(self._lib.sv_despeckle_u8(self._h, _ptr(binary), n, H, W, _ptr(out), _opt_ptr(packed),
                                                    _stream_ptr()), "sv_despeckle_u8")
        return out if packed is None else packed

    def component_filter_bits(self, bits, min_area_ratio=0.1):
        """component_filter on a bit image int32 [n,H,W//32], in place."""
        self._out(_dev_tensor(bits, "bits", torch.int32, self.device, ndim=3), bits.shape, torch.int32, "bits")
        n, H, wpr = bits.shape
        if not float(min_area_ratio) >= 0:
            raise ValueError(f"min_area_ratio must be >= 0, got {min_area_ratio}")
        if n == 0:                                                 # an empty tensor has no pointer to pass
            return bits
        self._check(self._lib.sv_component_filter_bits(self._h, _ptr(bits), n, H, wpr * 32, float(min_area_ratio), _stream_ptr()), "sv_component_filter_bits")
        return bits

    def component_filter(self, binary, min_area_ratio=0.1, out=None, packed=None):
        """binary u8 [n,H,W] (foreground = non-zero) -> the same with every 8-connected component erased whose bounding box has
        (x1 - x0) * (y1 - y0) < min_area_ratio * H * W: exactly those, whatever their shape (sv_component_filter_u8 in the header).
        host.find_grid_corners of the result equals that of `binary` for every search ratio >= min_area_ratio.  out may be binary;
        packed: optional int32 [n,H,W//32] tensor that also receives the result as 1 bit per pixel (W % 32 == 0)."""
        binary = _dev_tensor(binary, "binary", torch.uint8, self.device, ndim=3).contiguous()
        n, H, W = binary.shape
        if not float(min_area_ratio) >= 0:
            raise ValueError(f"min_area_ratio must be >= 0, got {min_area_ratio}")
        out = self._out(out, (n, H, W), torch.uint8, "out")
        if packed is not None:
            if W % 32:
                raise ValueError("packed needs W % 32 == 0")
            self._out(packed, (n, H, W // 32), torch.int32, "packed")
        if n == 0:
            return out
        self._check(self._lib.sv_component_filter_u8(self._h, _ptr(binary), n, H, W, float(min_area_ratio), _ptr(out), _opt_ptr(packed),
                                                     _stream_ptr()), "sv_component_filter_u8")
        return out

    def pack_sparse_bits(self, bits, records):
        """bits int32 [n,H,W//32] (despeckle's packed output) -> records uint8 [n,stride] (device): per frame the row masks of its
        non-zero words and those words (sv_pack_sparse_bits; layout in include/sudoku_vision_hip.h).  A third to a quarter of the
        dense image for the D2H copy; host.find_grid_corners_sparse_batch reads it."""
        _dev_tensor(bits, "bits", torch.int32, self.device, ndim=3)
        _dev_tensor(records, "records", torch.uint8, self.device, ndim=2)
        n, H, wpr = bits.shape
        if records.shape[0] < n or not records.is_contiguous() or not bits.is_contiguous():
            raise TypeError("records must be a contiguous uint8 [>=n, stride] device tensor")
        self._check(self._lib.sv_pack_sparse_bits(self._h, _ptr(bits), n, H, wpr * 32, _ptr(records), records.shape[1], _stream_ptr()),
                      "sv_pack_sparse_bits")
        return records[:n]

    def copy_to_pinned(self, src, dst):
        """src (device tensor) -> dst (pinned host tensor of the same byte size) by a copy kernel on the current stream: about twice
        the PCIe rate of the DMA engine tensor.copy_(non_blocking=True) uses (sv_copy_to_pinned_host).  Stream-ordered; synchronise
        (an event, the stream) before reading dst."""
        _dev_tensor(src, "src", None, self.device)
        if not dst.is_pinned() or not dst.is_contiguous() or not src.is_contiguous():
            raise TypeError("copy_to_pinned needs a contiguous device tensor and a contiguous pinned host tensor")
        nbytes = src.numel() * src.element_size()
        if nbytes != dst.numel() * dst.element_size():
            raise ValueError("size mismatch")
        self._check(self._lib.sv_copy_to_pinned_host(self._h, _ptr(src), _ptr(dst), nbytes, _stream_ptr()), "sv_copy_to_pinned_host")
        return dst

    # ---- K2 -----------------------------------------------------------------------------------
    @staticmethod
    def corners_to_minv(corners, output_size=450, inset_ratio=0.0):
        """corners [n,4,2] (host, any order) -> float64 [n,3,3] destination->source homographies (host)."""
        c = np.ascontiguousarray(np.asarray(corners, dtype=np.float32).reshape(-1, 8))
        out = np.empty((c.shape[0], 3, 3), np.float64)
        _native.check(_native.lib().sv_corners_to_minv(c.ctypes.data_as(C.c_void_p), c.shape[0], int(output_size), float(inset_ratio),
                                                       out.ctypes.data_as(C.c_void_p)), "sv_corners_to_minv")
        return out

    @staticmethod
    def corners_to_minv_batch(corners, output_size=450, inset_ratio=0.0):
        """As corners_to_minv, but a degenerate quad does not raise: -> (minv float64 [n,3,3], ok bool [n]); minv[f] is the
        identity where ok[f] is False."""
        c = np.ascontiguousarray(np.asarray(corners, dtype=np.float32).reshape(-1, 8))
        out = np.empty((c.shape[0], 3, 3), np.float64)
        ok = np.empty(c.shape[0], np.uint8)
        _native.check(_native.lib().sv_corners_to_minv_batch(c.ctypes.data_as(C.c_void_p), c.shape[0], int(output_size), float(inset_ratio),
                                                             out.ctypes.data_as(C.c_void_p), ok.ctypes.data_as(C.c_void_p)), "sv_corners_to_minv_batch")
        return out, ok.astype(bool)

    @staticmethod
    def corners_to_m_batch(corners, output_size=450, inset_ratio=0.0):
        """The forward homographies of corners_to_minv_batch (sv_corners_to_m_batch): corners [n,4,2] (host, any order) ->
        (m float64 [n,3,3] frame -> grid, ok bool [n]); m[f] is the identity where ok[f] is False.  render_overlay takes them."""
        c = np.ascontiguousarray(np.asarray(corners, dtype=np.float32).reshape(-1, 8))
        out = np.empty((c.shape[0], 3, 3), np.float64)
        ok = np.empty(c.shape[0], np.uint8)
        _native.check(_native.lib().sv_corners_to_m_batch(c.ctypes.data_as(C.c_void_p), c.shape[0], int(output_size), float(inset_ratio),
                                                          out.ctypes.data_as(C.c_void_p), ok.ctypes.data_as(C.c_void_p)), "sv_corners_to_m_batch")
        return out, ok.astype(bool)

    def minv_to_device(self, minv):
        return torch.from_numpy(np.ascontiguousarray(minv, np.float64)).to(self.device)

    def warp_perspective(self, img, minv_dev, output_size):
        """img u8 [H,W] or [H,W,1|3] on device (rows may be padded: cropped views are read in place) -> the output_size square."""
        _dev_tensor(img, "img", torch.uint8, self.device, ndim=(2, 3))
        if img.dim() == 3 and img.shape[2] not in (1, 3):
            raise ValueError(f"img must have 1 or 3 channels, got {list(img.shape)}")
        minv_dev = self._minv(minv_dev, 1)
        img, pitch = _image_layout(img)
        H, W = img.shape[0], img.shape[1]
        ch = 1 if img.dim() == 2 else img.shape[2]
        shape = (output_size, output_size) if img.dim() == 2 else (output_size, output_size, ch)
        out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        self._check(self._lib.sv_warp_perspective_u8(self._h, _ptr(img), H, W, pitch, ch, _ptr(minv_dev), int(output_size), _ptr(out),
                                                           _stream_ptr()), "sv_warp_perspective_u8")
        return out

    def extract_cells(self, grid, cell_size, margin_h, margin_w):
        """grid u8 [h,w] or [h,w,1|3] on device (rows may be padded) -> 81 cells u8 [81,cell_size,cell_size]."""
        _dev_tensor(grid, "grid", torch.uint8, self.device, ndim=(2, 3))
        if grid.dim() == 3 and grid.shape[2] not in (1, 3):
            raise ValueError(f"grid must have 1 or 3 channels, got {list(grid.shape)}")
        grid, pitch = _image_layout(grid)
        h, w = grid.shape[0], grid.shape[1]
        ch = 1 if grid.dim() == 2 else grid.shape[2]
        out = torch.empty((81, cell_size, cell_size), dtype=torch.uint8, device=self.device)
        self._check(self._lib.sv_extract_cells_u8(self._h, _ptr(grid), h, w, pitch, ch, int(cell_size), int(margin_h), int(margin_w),
                                                        _ptr(out), _stream_ptr()), "sv_extract_cells_u8")
        return out

    def warp_cells(self, frames, minv_dev):
        frames, pitch, fstride = _frame_layout(frames, self.device)
        n, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
        minv_dev = self._minv(minv_dev, n)
        out = torch.empty((n, 81, 28, 28), dtype=torch.uint8, device=self.device)
        self._check(self._lib.sv_warp_cells_u8(self._h, _ptr(frames), n, H, W, pitch, fstride, _ptr(minv_dev), _ptr(out), _stream_ptr()),
                      "sv_warp_cells_u8")
        return out

    # ---- K3 -----------------------------------------------------------------------------------
    GLUE_NORMALIZE, GLUE_RUNPY = 0, 1

    def resize_linear(self, img, dsize):
        """cv2.resize(img, dsize=(w, h)) INTER_LINEAR on a gray u8 image."""
        img, pitch = _image_layout(_dev_tensor(img, "img", torch.uint8, self.device, ndim=2))
        dw, dh = dsize
        out = torch.empty((dh, dw), dtype=torch.uint8, device=self.device)
        self._check(self._lib.sv_resize_linear_u8(self._h, _ptr(img), img.shape[0], img.shape[1], pitch, _ptr(out), dh, dw, _stream_ptr()),
                      "sv_resize_linear_u8")
        return out

    def cell_ink_ratio(self, cells):
        """cells u8 [B,h,w] -> (ratio f32 [B], otsu i32 [B]): is_cell_empty's Otsu ink share, batched."""
        cells = _dev_tensor(cells, "cells", torch.uint8, self.device, ndim=3).contiguous()
        B = cells.shape[0]
        ratio = torch.empty((B,), dtype=torch.float32, device=self.device)
        otsu = torch.empty((B,), dtype=torch.int32, device=self.device)
        self._check(self._lib.sv_cell_ink_ratio_u8(self._h, _ptr(cells), B, int(cells[0].numel()), _ptr(ratio), _ptr(otsu), _stream_ptr()),
                      "sv_cell_ink_ratio_u8")
        return ratio, otsu

    # ---- JPEG front end (scope row N4) -----------------------------------------------------------------
    def _jpeg_staging(self, nbytes):
        """Two pinned + device staging sets used alternately, so the H2D copy and reconstruction of one call overlap the
        host Huffman decoding of the next.  Returns (pinned u8 tensor, device u8 tensor) of at least nbytes."""
        if not hasattr(self, "_jpeg_sets"):
            self._jpeg_sets, self._jpeg_turn = [None, None], 0
        self._jpeg_turn ^= 1
        cur = self._jpeg_sets[self._jpeg_turn]
        if cur is not None:
            cur[2].synchronize()                                       # the copy that last read this set has finished
        if cur is None or cur[0].numel() < nbytes:
            cap = int(nbytes * 1.25) + 4096
            cur = [torch.empty(cap, dtype=torch.uint8).pin_memory(), torch.empty(cap, dtype=torch.uint8, device=self.device), torch.cuda.Event()]
            self._jpeg_sets[self._jpeg_turn] = cur
        return cur

    @staticmethod
    def _jpeg_layout(info, base, dense):
        """Where one image's coefficients lie in a staging buffer, from byte offset `base`: ((masks, offsets, values, capacity in values),
        the 64-byte aligned end).  dense: plain int16 blocks, no masks or offsets."""
        ncoef, nb = int(info.coef_count), int(info.coef_count) // 64
        if dense:
            return (0, 0, base, ncoef), base + (2 * ncoef + 63) // 64 * 64
        cap = int(info.sparse_capacity)
        return (base, base + 8 * nb, base + 12 * nb, cap), base + (12 * nb + 2 * cap + 63) // 64 * 64

    def _jpeg_reconstruct(self, info, db, lay, qoff, out, dense, stream, reduce=1, gray=False):
        """Coefficients staged at device address db as _jpeg_layout `lay`, quantisation tables at db + qoff -> BGR in `out`, on `stream`.
        gray: Y's records alone (info from sv_jpeg_parse_luma) -> the [H,W] image in `out`."""
        p = [C.c_void_p(db + lay[2])] if dense else [C.c_void_p(db + o) for o in lay[:3]]
        args = (self._h, C.byref(info), *p, C.c_void_p(db + qoff), _ptr(out), out.stride(0), stream)
        if gray:
            fn = self._lib.sv_jpeg_reconstruct_gray_u8 if dense else self._lib.sv_jpeg_reconstruct_sparse_gray_u8
            self._check(fn(*args, reduce), "sv_jpeg_reconstruct_gray")
        elif reduce == 1:
            fn = self._lib.sv_jpeg_reconstruct_bgr_u8 if dense else self._lib.sv_jpeg_reconstruct_sparse_bgr_u8
            self._check(fn(*args), "sv_jpeg_reconstruct")
        else:
            fn = self._lib.sv_jpeg_reconstruct_scaled_bgr_u8 if dense else self._lib.sv_jpeg_reconstruct_sparse_scaled_bgr_u8
            self._check(fn(*args, reduce), "sv_jpeg_reconstruct_scaled")

    @staticmethod
    def jpeg_reduce_arg(reduce):
        """reduce= of the imdecode family: libjpeg's scale_denom, 1, 2, 4 or 8"""
        if not isinstance(reduce, (int, np.integer)) or reduce not in (1, 2, 4, 8):
            raise ValueError(f"reduce must be 1, 2, 4 or 8, not {reduce!r}")
        return int(reduce)

    def _jpeg_out_shape(self, info, reduce):
        """(rows, columns) of the decoded frame: ceil(out_height / reduce), ceil(out_width / reduce)"""
        w, h = C.c_int(), C.c_int()
        self._check(self._lib.sv_jpeg_scaled_size(C.byref(info), reduce, C.byref(w), C.byref(h)), "sv_jpeg_scaled_size")
        return h.value, w.value

    def imdecode_batch(self, datas, threads=16, dense=False, reduce=1, gray=False):
        """A batch of JPEG files -> uint8 CUDA tensor [n,H,W,3] when all share a shape, else a list of [H,W,3] tensors.
        reduce = 2, 4 or 8 (one value for the batch): libjpeg's reduced-size decode, frames of ceil(H / reduce) x ceil(W / reduce).
        gray=True: cv2.IMREAD_GRAYSCALE / IMREAD_REDUCED_GRAYSCALE_*, [n,H,W] or a list of [H,W]: the luma-only decode -- only Y's
        coefficients are stored, staged and copied, and one kernel (csrc/k20_jpeg_gray.hip) writes the image; colour and gray-only files mix.
        Images are Huffman-decoded on `threads` host threads (sv_jpeg_entropy_decode_batch) into pinned memory in the compact
        mask + values form (dense=True: plain int16 blocks), cross PCIe one image per copy, and are reconstructed on the GPU
        back to back.  Returns after the last launch; the next call's host decoding overlaps this call's copies and kernels."""
        from . import host
        reduce = self.jpeg_reduce_arg(reduce)
        n = len(datas)
        datas = [bytes(d) for d in datas]
        infos = [(host.jpeg_parse_luma if gray else host.jpeg_parse)(d) for d in datas]
        ch, qbytes = ((), 128) if gray else ((3,), 384)                # Y's quantiser steps alone, or three components'
        base, lay, total = [], [], 0
        for info in infos:
            base.append(total)
            l, total = self._jpeg_layout(info, total, dense)
            lay.append(l)
        qoff = total
        total += qbytes * n
        pin, dev, ev = self._jpeg_staging(total)
        pb, db = pin.data_ptr(), dev.data_ptr()
        VP = C.c_void_p * n
        bufs = (C.c_char_p * n)(*datas)
        sizes = (C.c_size_t * n)(*[len(d) for d in datas])
        status = (C.c_int * n)()
        used = (C.c_long * n)()
        if dense:
            args = (VP(*[pb + l[2] for l in lay]), None, None, None, None, None)
        else:
            args = (None, VP(*[pb + l[0] for l in lay]), VP(*[pb + l[1] for l in lay]), VP(*[pb + l[2] for l in lay]),
                    (C.c_long * n)(*[l[3] for l in lay]), used)
        decode = self._lib.sv_jpeg_entropy_decode_luma_batch if gray else self._lib.sv_jpeg_entropy_decode_batch
        self._check(decode(bufs, sizes, n, *args, C.c_void_p(pb + qoff), int(threads), status), "sv_jpeg_entropy_decode_luma_batch" if gray else "sv_jpeg_entropy_decode_batch")
        shapes = [self._jpeg_out_shape(i, reduce) for i in infos]
        same = all(sh == shapes[0] for sh in shapes)
        if same:
            out = torch.empty((n, *shapes[0], *ch), dtype=torch.uint8, device=self.device)
            outs = [out[i] for i in range(n)]
        else:
            outs = [torch.empty((*sh, *ch), dtype=torch.uint8, device=self.device) for sh in shapes]
        dev[qoff:qoff + qbytes * n].copy_(pin[qoff:qoff + qbytes * n], non_blocking=True)
        sent, stream = 0, _stream_ptr()
        for i, (info, l) in enumerate(zip(infos, lay)):
            end = l[2] + 2 * (int(info.coef_count) if dense else used[i])
            dev[base[i]:end].copy_(pin[base[i]:end], non_blocking=True)
            self._jpeg_reconstruct(info, db, l, qoff + qbytes * i, outs[i], dense, stream, reduce, gray)
            sent += end - base[i]
        ev.record(torch.cuda.current_stream(self.device))
        self._jpeg_last_bytes = sent / max(n, 1)
        return out if same else outs

    def imdecode(self, data: bytes, threads=1, out=None, dense=False, reduce=1, gray=False):
        """cv2.imdecode / cv2.imread of a baseline JPEG -> BGR uint8 CUDA tensor [H,W,3] (EXIF orientation applied).
        Huffman decoding on the host (csrc/host_jpeg.cpp; `threads` work on restart intervals when the file has them) into
        pinned staging memory, everything after it on the GPU.  reduce = 2, 4 or 8: cv2.IMREAD_REDUCED_COLOR_*, the frame is
        ceil(H / reduce) x ceil(W / reduce) and is never reconstructed at full size.
        gray=True: cv2.IMREAD_GRAYSCALE / IMREAD_REDUCED_GRAYSCALE_*, a [H,W] tensor: libjpeg's JCS_GRAYSCALE, the inverse DCT of Y alone
        (not the gray conversion of the colour image).  out= may be a view whose rows are dense (stride(1) == 1): it is written by its pitch."""
        reduce = self.jpeg_reduce_arg(reduce)
        if out is None and threads <= 1:
            return self.imdecode_batch([data], 1, dense=dense, reduce=reduce, gray=gray)[0]
        from . import host
        data = bytes(data)
        info = (host.jpeg_parse_luma if gray else host.jpeg_parse)(data)
        lay, qoff = self._jpeg_layout(info, 0, dense)
        pin, dev, ev = self._jpeg_staging(qoff + 384)
        pb, db = pin.data_ptr(), dev.data_ptr()
        if dense:
            decode = self._lib.sv_jpeg_entropy_decode_luma if gray else self._lib.sv_jpeg_entropy_decode
            self._check(decode(data, len(data), C.c_void_p(pb), C.c_void_p(pb + qoff), int(threads)), "sv_jpeg_entropy_decode")
            end = 2 * int(info.coef_count)
        else:
            used = C.c_long()
            decode = self._lib.sv_jpeg_entropy_decode_luma_sparse if gray else self._lib.sv_jpeg_entropy_decode_sparse
            self._check(decode(data, len(data), *[C.c_void_p(pb + o) for o in lay[:3]], lay[3], C.byref(used), C.c_void_p(pb + qoff), int(threads)),
                        "sv_jpeg_entropy_decode_sparse")
            end = lay[2] + 2 * used.value
        dev[:end].copy_(pin[:end], non_blocking=True)
        dev[qoff:qoff + 384].copy_(pin[qoff:qoff + 384], non_blocking=True)
        shape = self._jpeg_out_shape(info, reduce)
        want = shape if gray else (*shape, 3)
        if out is None:
            out = torch.empty(want, dtype=torch.uint8, device=self.device)
        elif tuple(out.shape) != want:
            raise ValueError(f"out must be {list(want)}, not {list(out.shape)}")
        elif gray and (out.dtype != torch.uint8 or not out.is_cuda or (out.shape[1] > 1 and out.stride(1) != 1) or out.stride(0) < out.shape[1]):
            raise ValueError("out must be a uint8 CUDA tensor whose rows are dense (a column-offset view of a wider tensor is fine)")
        self._jpeg_reconstruct(info, db, lay, qoff, out, dense, _stream_ptr(), reduce, gray)
        ev.record(torch.cuda.current_stream(self.device))
        return out

    # ---- JPEG encoder (cv2.imwrite, pipeline/run.py:431) -----------------------------------------------
    JPEG_SAMPLINGS = {"444": 0, "422": 1, "420": 2}
    _ENC_CHUNK_BYTES = 128 << 20                                       # device staging of one chunk of an imencode_batch

    def jpeg_encode_plan(self, width, height, channels, quality=95, sampling="420", restart=0):
        """sv_jpeg_encode_plan, cached: the geometry, quantiser tables and size bounds of one (shape, quality, sampling, restart).
        ValueError for what the encoder does not write."""
        if not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
            raise ValueError(f"quality must be an integer in 1..100, not {quality!r}")
        if str(sampling) not in self.JPEG_SAMPLINGS:
            raise ValueError(f"sampling must be '444', '422' or '420', not {sampling!r}")
        if not isinstance(restart, (int, np.integer)) or not 0 <= restart <= 65535:
            raise ValueError(f"restart must be an integer in 0..65535 (MCUs), not {restart!r}")
        if channels not in (1, 3) or not (0 < width < 65536 and 0 < height < 65536):
            raise ValueError(f"cannot encode a {height} x {width} image of {channels} channels")
        key = (int(width), int(height), int(channels), int(quality), str(sampling), int(restart))
        plans = self.__dict__.setdefault("_jpeg_plans", {})
        if key not in plans:
            plan = _native.JpegEnc()
            self._check(self._lib.sv_jpeg_encode_plan(*key[:3], self.JPEG_SAMPLINGS[key[4]], key[3], key[5], C.byref(plan)), "sv_jpeg_encode_plan")
            plans[key] = plan
        return plans[key]

    def _enc_frames(self, frames):
        """frames of an encode call -> (u8 tensor [n,H,W,3] or [n,H,W] on this device, channels).  A list is stacked; a tensor, views and padded
        rows included, is passed on as it is (the kernel reads any row pitch)."""
        if isinstance(frames, (list, tuple)):
            if not frames:
                raise ValueError("no frames")
            for f in frames:
                _dev_tensor(f, "frames[i]", torch.uint8, self.device, ndim=(2, 3))
            if any(f.shape != frames[0].shape for f in frames):
                raise ValueError("the frames of a batch share a shape (a batch shares its plan)")
            frames = torch.stack(list(frames))
        _dev_tensor(frames, "frames", torch.uint8, self.device, ndim=(3, 4))
        if frames.dim() == 4 and frames.shape[3] != 3:
            raise ValueError(f"colour frames are [n,H,W,3] BGR, got {list(frames.shape)}")
        if frames.numel() == 0:
            raise ValueError(f"empty frames {list(frames.shape)}")
        return frames, 3 if frames.dim() == 4 else 1

    def jpeg_forward(self, frames, plan, dense=False):
        """The device half alone (sv_jpeg_forward_bgr_u8 / _gray_u8) on the current stream.  dense: int16 [n, coef_count] in the decoder's layout.
        Otherwise the sparse transport form: (masks u64 [n, blocks], offsets u32 [n, blocks], values i16 [n, coef_count], counts u32 [n])."""
        frames, ch = self._enc_frames(frames)
        x, pitch, stride = _batch_layout(frames, self.device, "frames", ch)
        n, ncoef = x.shape[0], int(plan.info.coef_count)
        if (plan.info.height, plan.info.width, plan.info.components) != (x.shape[1], x.shape[2], ch):
            raise ValueError("the plan was made for another shape")
        fn = self._lib.sv_jpeg_forward_bgr_u8 if ch == 3 else self._lib.sv_jpeg_forward_gray_u8
        if dense:
            coef = torch.empty((n, ncoef), dtype=torch.int16, device=self.device)
            self._check(fn(self._h, C.byref(plan), _ptr(x), n, pitch, stride, _ptr(coef), None, None, None, None, _stream_ptr()), "sv_jpeg_forward")
            return coef
        masks = torch.empty((n, ncoef // 64), dtype=torch.int64, device=self.device)
        offsets = torch.empty((n, ncoef // 64), dtype=torch.int32, device=self.device)
        values = torch.empty((n, ncoef), dtype=torch.int16, device=self.device)
        counts = torch.empty((n,), dtype=torch.int32, device=self.device)
        self._check(fn(self._h, C.byref(plan), _ptr(x), n, pitch, stride, None, _ptr(masks), _ptr(offsets), _ptr(values), _ptr(counts), _stream_ptr()), "sv_jpeg_forward")
        return masks, offsets, values, counts

    def _enc_pinned(self, nbytes):
        cur = getattr(self, "_enc_pin", None)
        if cur is None or cur.numel() < nbytes:
            self._enc_pin = cur = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8).pin_memory()
        return cur

    def imencode_batch(self, frames, quality=95, sampling="420", restart=0, threads=1):
        """cv2.imencode('.jpg', frame)[1].tobytes() for every frame of a uint8 CUDA batch [n,H,W,3] (BGR) or [n,H,W] (gray), or a list of
        same-shaped frames -> list of bytes, each the file libjpeg-turbo writes (baseline, Annex K tables, JFIF header; cv2's defaults are quality
        95 and 4:2:0).  The GPU computes the quantised coefficients in the compact mask + values form (csrc/k17_jpeg_encode.hip), only
        the used part of which crosses PCIe into pinned memory; `threads` host threads pack the Huffman bit streams (csrc/host_jpeg.cpp),
        one image each.  restart: MCUs per restart interval (0: none).  Synchronises the current stream."""
        frames, ch = self._enc_frames(frames)
        n, H, W = frames.shape[:3]
        plan = self.jpeg_encode_plan(W, H, ch, quality, sampling, restart)
        ncoef, nb = int(plan.info.coef_count), int(plan.info.coef_count) // 64
        step = max(1, min(n, self._ENC_CHUNK_BYTES // (12 * nb + 4 * ncoef)))
        stream = torch.cuda.current_stream(self.device)
        out = []
        for at in range(0, n, step):
            m = min(step, n - at)
            masks, offsets, values, counts = self.jpeg_forward(frames[at:at + m], plan)
            cb = (4 * m + 63) // 64 * 64                               # counts, then the masks and the offsets of the chunk
            head = cb + 12 * nb * m
            pin = self._enc_pinned(head)
            pin[:4 * m].view(torch.int32).copy_(counts, non_blocking=True)
            pin[cb:cb + 8 * nb * m].view(torch.int64).copy_(masks.view(-1), non_blocking=True)
            pin[cb + 8 * nb * m:head].view(torch.int32).copy_(offsets.view(-1), non_blocking=True)
            stream.synchronize()
            used = [int(c) for c in pin[:4 * m].view(torch.int32).tolist()]
            starts = np.concatenate([[0], np.cumsum([2 * u + 2 for u in used])]).astype(np.int64) + head       # never an empty stretch
            if pin.numel() < starts[-1]:
                keep = pin[:head].clone()
                pin = self._enc_pinned(int(starts[-1]))
                pin[:head].copy_(keep)
            for i, u in enumerate(used):
                if u:
                    pin[int(starts[i]):int(starts[i]) + 2 * u].view(torch.int16).copy_(values[i, :u], non_blocking=True)
            stream.synchronize()
            pb = pin.data_ptr()
            bounds = [int(self._lib.sv_jpeg_encode_bound(C.byref(plan), u)) for u in used]
            bufs = [np.empty(b, np.uint8) for b in bounds]
            VP = C.c_void_p * m
            sizes, status = (C.c_size_t * m)(), (C.c_int * m)()
            self._check(self._lib.sv_jpeg_entropy_encode_batch(
                C.byref(plan), m, VP(*[pb + cb + 8 * nb * i for i in range(m)]), VP(*[pb + cb + 8 * nb * m + 4 * nb * i for i in range(m)]),
                VP(*[pb + int(s) for s in starts[:m]]), (C.c_long * m)(*used), VP(*[b.ctypes.data for b in bufs]), (C.c_size_t * m)(*bounds), sizes,
                int(threads), status), "sv_jpeg_entropy_encode_batch")
            out += [bufs[i][:sizes[i]].tobytes() for i in range(m)]
        return out

    def imencode(self, frame, quality=95, sampling="420", restart=0, threads=1):
        """One uint8 CUDA frame [H,W,3] (BGR) or [H,W] (gray), any row pitch -> the bytes of its JPEG file (imencode_batch of one frame; `threads`
        work on restart intervals when restart > 0)."""
        _dev_tensor(frame, "frame", torch.uint8, self.device, ndim=(2, 3))
        return self.imencode_batch(frame[None], quality, sampling, restart, threads)[0]

    # ---- PNG encoder (cv2.imwrite of a .png path: pipeline/run.py --output solved.png, tools/extract_cells.py) ------------------------
    PNG_FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}
    PNG_STRATEGIES = {"rle": 0, "huffman_only": 1, "stored": 2}

    def png_encode_plan(self, width, height, channels, filter="sub", strategy="rle", band_rows=0):
        """sv_png_encode_plan, cached: the bands and size bounds of one (shape, filter, strategy, band_rows).  band_rows 0: automatic.
        ValueError for what the encoder does not write."""
        if str(filter) not in self.PNG_FILTERS:
            raise ValueError(f"filter must be one of {sorted(self.PNG_FILTERS)}, not {filter!r}")
        if str(strategy) not in self.PNG_STRATEGIES:
            raise ValueError(f"strategy must be one of {sorted(self.PNG_STRATEGIES)}, not {strategy!r}")
        if not isinstance(band_rows, (int, np.integer)) or band_rows < 0:
            raise ValueError(f"band_rows must be a non-negative integer, not {band_rows!r}")
        if channels not in (1, 3) or not (0 < width < 65536 and 0 < height < 65536):
            raise ValueError(f"cannot encode a {height} x {width} image of {channels} channels")
        key = (int(width), int(height), int(channels), str(filter), str(strategy), int(band_rows))
        plans = self.__dict__.setdefault("_png_plans", {})
        if key not in plans:
            plan = _native.PngEnc()
            self._check(self._lib.sv_png_encode_plan(*key[:3], self.PNG_FILTERS[key[3]], self.PNG_STRATEGIES[key[4]], key[5], C.byref(plan)), "sv_png_encode_plan")
            plans[key] = plan
        return plans[key]

    def png_deflate(self, frames, plan):
        """The device half alone (sv_png_deflate_bgr_u8 / _gray_u8) on the current stream: (stream u8 [n, stream_bound], band_len u32 [n, bands],
        adler u32 [n, bands], status u32 [n, bands]).  Frame f's bands lie back to back at the start of stream[f]; sum(band_len[f]) bytes count."""
        frames, ch = self._enc_frames(frames)
        x, pitch, stride = _batch_layout(frames, self.device, "frames", ch)
        n = x.shape[0]
        if x.shape[1] == 1:
            pitch = max(pitch, x.shape[2] * ch)                        # the stride of a one-row dimension is whatever the view left there
        if (plan.height, plan.width, plan.channels) != (x.shape[1], x.shape[2], ch):
            raise ValueError("the plan was made for another shape")
        stream = torch.empty((n, int(plan.stream_bound)), dtype=torch.uint8, device=self.device)
        band_len, adler, status = (torch.empty((n, int(plan.bands)), dtype=torch.int32, device=self.device) for _ in range(3))
        fn = self._lib.sv_png_deflate_bgr_u8 if ch == 3 else self._lib.sv_png_deflate_gray_u8
        self._check(fn(self._h, C.byref(plan), _ptr(x), n, pitch, stride, _ptr(stream), _ptr(band_len), _ptr(adler), _ptr(status), _stream_ptr()), "sv_png_deflate")
        return stream, band_len, adler, status

    def imencode_png_batch(self, frames, filter="sub", strategy="rle", threads=1, band_rows=0):
        """cv2.imencode('.png', frame)[1].tobytes() for every frame of a uint8 CUDA batch [n,H,W,3] (BGR) or [n,H,W] (gray), or a list of
        same-shaped frames -> list of bytes: 8-bit RGB or gray PNG files, IHDR + one IDAT + IEND.  Lossless; the pixels are what any PNG reader gives
        back, the bytes are this encoder's own (bands of rows compressed independently on the GPU, csrc/k18_png_encode.hip).  The defaults are
        cv2's: the Sub filter and distance-1 matches (Z_RLE).  Only the compressed bytes and the bands' lengths cross PCIe; `threads` host
        threads add the container and the checksums (csrc/host_png.cpp), one image each.  Synchronises the current stream."""
        frames, ch = self._enc_frames(frames)
        n, H, W = frames.shape[:3]
        plan = self.png_encode_plan(W, H, ch, filter, strategy, band_rows)
        bands, bound = int(plan.bands), int(plan.stream_bound)
        step = max(1, min(n, self._ENC_CHUNK_BYTES // (bound + 12 * bands)))
        stream = torch.cuda.current_stream(self.device)
        out = []
        for at in range(0, n, step):
            m = min(step, n - at)
            data, band_len, adler, status = self.png_deflate(frames[at:at + m], plan)
            head = 12 * bands * m                                      # the lengths, Adler sums and statuses of the chunk
            pin = self._enc_pinned(head)
            for k, t in enumerate((band_len, adler, status)):
                pin[4 * bands * m * k:4 * bands * m * (k + 1)].view(torch.int32).copy_(t.view(-1), non_blocking=True)
            stream.synchronize()
            meta = pin[:head].view(torch.int32).numpy().view(np.uint32).reshape(3, m, bands).copy()
            if meta[2].any():
                raise _native.NativeError("sv_png_deflate: a band did not fit its slot")
            used = meta[0].sum(axis=1, dtype=np.int64)
            starts = np.concatenate([[0], np.cumsum(used + 1)]).astype(np.int64)                               # never an empty stretch
            pin = self._enc_pinned(int(starts[-1]))
            for i in range(m):
                if used[i]:
                    pin[int(starts[i]):int(starts[i] + used[i])].copy_(data[i, :int(used[i])], non_blocking=True)
            stream.synchronize()
            pb = pin.data_ptr()
            bufs = [np.empty(int(u) + 80, np.uint8) for u in used]
            VP = C.c_void_p * m
            sizes, rcs = (C.c_size_t * m)(), (C.c_int * m)()
            self._check(self._lib.sv_png_assemble_batch(
                C.byref(plan), m, VP(*[pb + int(s) for s in starts[:m]]), VP(*[meta[0, i].ctypes.data for i in range(m)]), VP(*[meta[1, i].ctypes.data for i in range(m)]),
                VP(*[b.ctypes.data for b in bufs]), (C.c_size_t * m)(*[b.size for b in bufs]), sizes, int(threads), rcs), "sv_png_assemble_batch")
            out += [bufs[i][:sizes[i]].tobytes() for i in range(m)]
        return out

    def imencode_png(self, frame, filter="sub", strategy="rle", threads=1, band_rows=0):
        """One uint8 CUDA frame [H,W,3] (BGR) or [H,W] (gray), any row pitch -> the bytes of its PNG file (imencode_png_batch of one frame)."""
        _dev_tensor(frame, "frame", torch.uint8, self.device, ndim=(2, 3))
        return self.imencode_png_batch(frame[None], filter, strategy, threads, band_rows)[0]

    # ---- PNG decoder (cv2.imread of a .png path: pipeline/run.py:250, tools/extract_cells.py's files read back) -------------------------
    _PNG_CHUNK_BYTES = 512 << 20                                       # filtered bytes staged per set of launches of an imdecode_png_batch

    def png_reconstruct(self, info, filtered, row_filter, palette=None, out=None, *, gray=False):
        """The device half alone (sv_png_reconstruct_bgr_u8) on the current stream.  filtered u8 [n, filtered_bytes], row_filter u8 [n, height],
        palette u8 [n, 1024] (colour type 3) on the device -> (out u8 [n,H,W,3], status i32 [n]); status[i] & 1: image i held a palette index past
        its palette's end.  out: a caller's [n,H,W,3] view with dense pixels (row padding and gaps between frames are left untouched).
        gray=True: sv_png_reconstruct_gray_u8, the IMREAD_GRAYSCALE read; out is then u8 [n,H,W]."""
        n, H, W = filtered.shape[0], int(info.height), int(info.width)
        ch = 1 if gray else 3
        _dev_tensor(filtered, "filtered", torch.uint8, self.device, shape=(n, int(info.filtered_bytes)))
        _dev_tensor(row_filter, "row_filter", torch.uint8, self.device, shape=(n, H))
        if palette is not None:
            _dev_tensor(palette, "palette", torch.uint8, self.device, shape=(n, _native.PNG_PALETTE_STRIDE))
        if not (filtered.is_contiguous() and row_filter.is_contiguous() and (palette is None or palette.is_contiguous())):
            raise ValueError("filtered, row_filter and palette must be contiguous")
        shape = (n, H, W) if gray else (n, H, W, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        _dev_tensor(out, "out", torch.uint8, self.device, shape=shape)
        st = out.stride()
        pitch = st[1] if H > 1 else max(st[1], ch * W)
        stride = st[0] if n > 1 else pitch * H
        if (not gray and st[3] != 1) or st[2] != ch or pitch < ch * W or (n > 1 and stride < pitch * (H - 1) + ch * W):
            raise ValueError(f"out must be a {list(shape)} view with dense pixels and rows and frames that do not overlap")
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        fn, name = (self._lib.sv_png_reconstruct_gray_u8, "sv_png_reconstruct_gray_u8") if gray else (self._lib.sv_png_reconstruct_bgr_u8, "sv_png_reconstruct_bgr_u8")
        self._check(fn(self._h, C.byref(info), _ptr(filtered), _ptr(row_filter), _opt_ptr(palette), n, _ptr(out), pitch, stride, _ptr(status), _stream_ptr()), name)
        return out, status

    def imdecode_png_batch(self, datas, threads=16, out=None, *, gray=False):
        """PNG files of ONE geometry (size, bit depth, colour type; anything else is a ValueError) -> uint8 CUDA tensor [n,H,W,3], each frame what
        cv2.imdecode(buf, IMREAD_COLOR) returns; gray=True: [n,H,W], what cv2.imdecode(buf, IMREAD_GRAYSCALE) returns (colour files: see
        sv_png_reconstruct_gray_u8).  `threads` host threads inflate into pinned memory (csrc/host_png.cpp), the filtered bytes cross
        PCIe in one copy and one set of launches unfilters and expands them (csrc/k19_png_decode.hip); batches above 512 MiB of filtered bytes go
        in several such sets.  NativeError for a file that is malformed (SV_ERR_BAD_ARG) or not decoded here (SV_ERR_UNSUPPORTED: Adam7).  Returns
        after the last launch, but for palette files, whose indices the GPU checks: those synchronise the current stream."""
        from . import host
        datas = [bytes(d) for d in datas]
        n = len(datas)
        if n == 0:
            raise ValueError("imdecode_png_batch needs at least one file")
        infos = [host.png_parse(d) for d in datas]
        info = infos[0]
        key = lambda i: (i.width, i.height, i.bit_depth, i.color_type)
        if any(key(i) != key(info) for i in infos):
            raise ValueError("imdecode_png_batch: the files differ in size, bit depth or colour type")
        H, W, fb, ps = int(info.height), int(info.width), int(info.filtered_bytes), _native.PNG_PALETTE_STRIDE
        shape = (n, H, W) if gray else (n, H, W, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        _dev_tensor(out, "out", torch.uint8, self.device, shape=shape)
        paletted = info.color_type == 3
        step = max(1, min(n, self._PNG_CHUNK_BYTES // (fb + H + ps)))
        stream = torch.cuda.current_stream(self.device)
        flags = []
        for at in range(0, n, step):
            m = min(step, n - at)
            rows_at = m * fb
            pal_at = (rows_at + m * H + 63) // 64 * 64
            total = pal_at + (m * ps if paletted else 0)
            pin, dev, ev = self._jpeg_staging(total)
            pb = pin.data_ptr()
            VP = C.c_void_p * m
            status = (C.c_int * m)()
            chunk = infos[at:at + m]
            self._check(self._lib.sv_png_inflate_batch((C.c_char_p * m)(*datas[at:at + m]), (C.c_size_t * m)(*[len(d) for d in datas[at:at + m]]),
                                                       (_native.PngInfo * m)(*chunk), m, VP(*[pb + i * fb for i in range(m)]), (C.c_size_t * m)(*([fb] * m)),
                                                       VP(*[pb + rows_at + i * H for i in range(m)]), int(threads), status), "sv_png_inflate_batch")
            pal = None
            if paletted:
                host_pal = pin[pal_at:total].numpy().reshape(m, ps)
                for i, inf in enumerate(chunk):
                    host_pal[i, :768] = np.frombuffer(bytes(inf.palette), np.uint8)
                    host_pal[i, 768:772] = np.frombuffer(np.uint32(inf.palette_entries).tobytes(), np.uint8)
                pal = dev[pal_at:total].view(m, ps)
            dev[:total].copy_(pin[:total], non_blocking=True)
            _, st = self.png_reconstruct(info, dev[:rows_at].view(m, fb), dev[rows_at:rows_at + m * H].view(m, H), pal, out[at:at + m], gray=gray)
            ev.record(stream)
            flags.append(st)
        if paletted:
            bad = torch.cat(flags).cpu()
            if bad.any():
                raise _native.NativeError(f"imdecode_png: SV_ERR_BAD_ARG: image {int(bad.nonzero()[0])} holds a palette index past its palette's end")
        return out

    def imdecode_png(self, data: bytes, threads=1, out=None, *, gray=False):
        """cv2.imdecode / cv2.imread of a PNG file -> BGR uint8 CUDA tensor [H,W,3] (imdecode_png_batch of one file; out: a [H,W,3] view);
        gray=True: the IMREAD_GRAYSCALE read, [H,W]."""
        return self.imdecode_png_batch([data], threads, None if out is None else out[None], gray=gray)[0]

    # ---- K24: a data set of PNG cells -> model input (ml/datasets.py:18-46, :69-92, :141-164; ml/evaluate.py:67) --------------------------------
    def dataset_cells(self, packed, mode="dataset", want=("f32",)):
        """One K24 launch over what host.dataset_pack made: one H2D copy of the packed bytes, then sv_dataset_cells on the current stream.
        mode "dataset" (datasets.preprocess_cell after the gray read) or "gray" (the gray read at 28 x 28 alone); want: "f32", "u8" or both.
        -> dict with "f32" f32 [n,1,28,28] and / or "u8" u8 [n,28,28], and "status" i32 [n] (bit 0: a palette index past the palette's end,
        bit 1: the kernel refused the record), all on the device.  Files dataset_pack could not pack (packed.status != 0) have their slot
        refused.  Does not synchronise."""
        modes = {"gray": _native.CELLS_GRAY, "dataset": _native.CELLS_DATASET}
        if mode not in modes:
            raise ValueError(f"mode must be 'gray' or 'dataset', got {mode!r}")
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(w not in ("f32", "u8") for w in want):
            raise ValueError(f"want must name 'f32', 'u8' or both, got {want!r}")
        n = packed.n
        dev = packed.pinned.to(self.device, non_blocking=True)
        out = {}
        if "u8" in want:
            out["u8"] = torch.empty((n, 28, 28), dtype=torch.uint8, device=self.device)
        if "f32" in want:
            out["f32"] = torch.empty((n, 1, 28, 28), dtype=torch.float32, device=self.device)
        out["status"] = torch.empty(n, dtype=torch.int32, device=self.device)
        # max(., 1): a pack without one decodable file still has a byte there, so that `filtered` is a pointer; every record is then refused
        self.dataset_cells_raw(dev[packed.filtered_at:packed.filtered_at + max(packed.filtered_size, 1)], dev[packed.records_at:packed.records_at + 16 * n],
                               dev[packed.palettes_at:packed.palettes_at + _native.PNG_PALETTE_STRIDE * packed.n_palettes] if packed.n_palettes else None,
                               modes[mode], out.get("u8"), out.get("f32"), out["status"])
        return out

    def dataset_cells_raw(self, filtered, records, palettes, mode, out_u8, out_f32, status):
        """sv_dataset_cells itself on the current stream, every argument a device tensor: filtered u8 [filtered_size], records u8 [16 n]
        (_native.DATASET_RECORD_DTYPE), palettes u8 [1024 k] or None, mode _native.CELLS_*, out_u8 u8 [n,28,28] or None, out_f32 f32 [n,1,28,28]
        or None, status i32 [n].  The kernel refuses what sv_dataset_check_records would; nothing here reads the records."""
        n = status.numel()
        _dev_tensor(filtered, "filtered", torch.uint8, self.device, ndim=1)
        _dev_tensor(records, "records", torch.uint8, self.device, shape=(16 * n,))
        _dev_tensor(status, "status", torch.int32, self.device, shape=(n,))
        if palettes is not None:
            _dev_tensor(palettes, "palettes", torch.uint8, self.device, ndim=1)
        if out_u8 is not None:
            self._out(out_u8, (n, 28, 28), torch.uint8, "out_u8")
        if out_f32 is not None:
            self._out(out_f32, (n, 1, 28, 28), torch.float32, "out_f32")
        if not (filtered.is_contiguous() and records.is_contiguous() and status.is_contiguous() and (palettes is None or palettes.is_contiguous())):
            raise ValueError("filtered, records, palettes and status must be contiguous")
        n_pal = 0 if palettes is None else palettes.numel() // _native.PNG_PALETTE_STRIDE
        self._check(self._lib.sv_dataset_cells(self._h, _ptr(filtered), filtered.numel(), _ptr(records), n, _opt_ptr(palettes), n_pal, int(mode), _opt_ptr(out_u8),
                                               _opt_ptr(out_f32), _ptr(status), _stream_ptr()), "sv_dataset_cells")

    def softmax_topk(self, logits, k=3):
        """F.softmax(logits, 1).topk(k) (pipeline/run_v2.py:165-178): (index u8 [B,k], prob f32 [B,k]), best first."""
        logits = _dev_tensor(logits, "logits", torch.float32, self.device).reshape(-1, 10).contiguous()
        B = logits.shape[0]
        index = torch.empty((B, k), dtype=torch.uint8, device=self.device)
        prob = torch.empty((B, k), dtype=torch.float32, device=self.device)
        self._check(self._lib.sv_softmax_topk_f32(self._h, _ptr(logits), B, int(k), _ptr(index), _ptr(prob), _stream_ptr()), "sv_softmax_topk_f32")
        return index, prob

    EVAL_OUTPUTS = {"probs": (torch.float32, (10,)), "pred": (torch.uint8, ()), "conf": (torch.float32, ()), "true_prob": (torch.float32, ()),
                    "nll": (torch.float32, ()), "correct": (torch.uint8, ())}
    EVAL_CONF_ONE = 1 << 30

    def eval_stats_buffer(self):
        """A zeroed sv_eval_stats block on the device, as int64 words (the counts are below 2^63): eval_metrics' `stats`."""
        return torch.zeros(C.sizeof(_native.EvalStats) // 8, dtype=torch.int64, device=self.device)

    @staticmethod
    def eval_stats_dict(stats, n_bins):
        """sv_eval_stats (an _native.EvalStats, or the int64 words of eval_stats_buffer, any device) -> plain dict of Python ints and
        lists; the confidence sums stay fixed point, in units of 1 / EVAL_CONF_ONE."""
        if isinstance(stats, torch.Tensor):
            stats = _native.EvalStats.from_buffer_copy(stats.cpu().numpy().tobytes())
        out = {"confusion": [[int(v) for v in row] for row in stats.confusion]}
        for k in ("n", "n_correct", "n_wrong", "bad_labels", "nonfinite"):
            out[k] = int(getattr(stats, k))
        for k in ("bin_count", "bin_correct", "bin_conf"):
            out[k] = [int(v) for v in getattr(stats, k)[:n_bins]]
        for k in ("tot_count", "tot_correct", "tot_conf"):
            out[k] = [int(v) for v in getattr(stats, k)]
        return out

    @staticmethod
    def eval_failures(failures, count):
        """The first `count` records of eval_metrics' failure buffer -> numpy structured array (fields of sv_eval_failure)."""
        raw = failures[:count].cpu().numpy().tobytes()
        return np.frombuffer(raw, dtype=_native.EVAL_FAILURE_DTYPE).copy()

    def eval_metrics(self, logits, labels, temperature=1.0, n_bins=10, max_failures=0, want=("pred", "conf", "correct"), *, probabilities=False,
                     bin_edges=None, stats=None, accumulate=False, index_base=0, failures=None, read_back=True):
        """Evaluation metrics of a batch in one pass (sv_eval_metrics; reference ml/evaluate_v2.py:67-220, ml/train.py:157-190).
        logits f32 [B,10] (probabilities=True: softmax outputs, compute_calibration's argument), labels int64 or int32 [B].
        -> (out, agg).  out: the device tensors named in `want` (EVAL_OUTPUTS), "stats" (the sv_eval_stats block, int64 words) and, with
        max_failures > 0, "failures" (u8 [max_failures,48], sv_eval_failure records: eval_failures decodes them).  agg: eval_stats_dict
        of the block after the call's one synchronisation -- or None with read_back=False, which reads nothing back and can be captured
        in a graph.  bin_edges: n_bins + 1 doubles, default np.linspace(0, 1, n_bins + 1).  stats / failures: buffers of an earlier call
        to go on with (accumulate=True keeps their contents; index_base is added to the failure records' sample index).
        A label outside 0..9 raises NativeError (SV_ERR_BAD_ARG) from the read-back form; `stats` then still holds every other cell."""
        logits = _dev_tensor(logits, "logits", torch.float32, self.device, shape=(None, 10)).contiguous()
        B = logits.shape[0]
        labels = _dev_tensor(labels, "labels", (torch.int64, torch.int32), self.device, shape=(B,)).contiguous()
        unknown = [k for k in want if k not in self.EVAL_OUTPUTS]
        if unknown:
            raise ValueError(f"want: unknown outputs {unknown}; known: {list(self.EVAL_OUTPUTS)}")
        n_bins, max_failures = int(n_bins), int(max_failures)
        edges = np.ascontiguousarray(np.linspace(0, 1, n_bins + 1) if bin_edges is None else bin_edges, dtype=np.float64)
        if edges.shape != (n_bins + 1,):
            raise ValueError(f"bin_edges must hold n_bins + 1 = {n_bins + 1} values, got shape {edges.shape}")
        out = {k: torch.empty((B,) + self.EVAL_OUTPUTS[k][1], dtype=self.EVAL_OUTPUTS[k][0], device=self.device) for k in want}
        words = C.sizeof(_native.EvalStats) // 8
        if stats is None:
            if accumulate:
                raise ValueError("accumulate=True needs the stats buffer of the calls before")
            stats = torch.empty(words, dtype=torch.int64, device=self.device)
        _dev_tensor(stats, "stats", torch.int64, self.device, shape=(words,))
        if max_failures > 0:
            if failures is None:
                failures = torch.empty((max_failures, _native.EVAL_FAILURE_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
            _dev_tensor(failures, "failures", torch.uint8, self.device, shape=(max_failures, _native.EVAL_FAILURE_DTYPE.itemsize))
        else:
            failures = None
        if not stats.is_contiguous() or (failures is not None and not failures.is_contiguous()):
            raise ValueError("stats and failures must be contiguous")
        args = [self._h, _ptr(logits), int(bool(probabilities)), _ptr(labels), int(labels.dtype == torch.int64), B, int(index_base), float(temperature),
                edges.ctypes.data_as(C.c_void_p), n_bins, int(bool(accumulate))] + [_opt_ptr(out.get(k)) for k in self.EVAL_OUTPUTS] + \
               [_ptr(stats), _opt_ptr(failures), max_failures]
        out["stats"] = stats
        if failures is not None:
            out["failures"] = failures
        if not read_back:
            self._check(self._lib.sv_eval_metrics(*args, _stream_ptr()), "sv_eval_metrics")
            return out, None
        host = _native.EvalStats()
        self._check(self._lib.sv_eval_metrics_host(*args, C.byref(host), _stream_ptr()), "sv_eval_metrics_host")
        return out, self.eval_stats_dict(host, n_bins)

    def preprocess_cells(self, cells):
        """run.py's preprocess_cell on u8 cells [B,28,28] -> u8 {0,255} [B,28,28]."""
        cells = _dev_tensor(cells, "cells", torch.uint8, self.device, shape=(None, 28, 28)).contiguous()
        out = torch.empty_like(cells)
        self._check(self._lib.sv_preprocess_cells_u8(self._h, _ptr(cells), cells.shape[0], _ptr(out), _stream_ptr()), "sv_preprocess_cells_u8")
        return out

    def _cnn_args(self, x, want_digits):
        """The argument of a CNN forward, checked: x f32 [B,1,28,28] or u8 [B,28,28] cells on this device -> (x contiguous, logits [B,10],
        digits u8 [B], conf f32 [B]); digits and conf are None unless wanted."""
        _dev_tensor(x, "x", (torch.uint8, torch.float32), self.device)
        if x.dtype == torch.uint8:
            _dev_tensor(x, "x", torch.uint8, self.device, shape=(None, 28, 28))
        elif not (x.dim() in (3, 4) and tuple(x.shape[-2:]) == (28, 28) and (x.dim() == 3 or x.shape[1] == 1)):
            raise ValueError(f"x must have shape [B,1,28,28], got {list(x.shape)}")
        B = x.shape[0]
        logits = torch.empty((B, 10), dtype=torch.float32, device=self.device)
        digits = torch.empty((B,), dtype=torch.uint8, device=self.device) if want_digits else None
        conf = torch.empty((B,), dtype=torch.float32, device=self.device) if want_digits else None
        return x.contiguous(), logits, digits, conf

    def cnn_forward(self, x, want_digits=False, glue=0):
        """x f32 [B,1,28,28], or u8 [B,28,28] cells with the run.py glue fused in (glue=GLUE_NORMALIZE: invert+normalise;
        GLUE_RUNPY: preprocess_cell (CLAHE + adaptive threshold) first) -> logits [B,10] (, digits, conf)."""
        x, logits, digits, conf = self._cnn_args(x, want_digits)
        B = x.shape[0]
        if x.dtype == torch.uint8:
            rc = self._lib.sv_cnn_forward_cells_u8(self._h, _ptr(x), B, int(glue), _ptr(logits), _opt_ptr(digits), _opt_ptr(conf), _stream_ptr())
        else:
            rc = self._lib.sv_cnn_forward_f32(self._h, _ptr(x), B, _ptr(logits), _opt_ptr(digits), _opt_ptr(conf), _stream_ptr())
        self._check(rc, "sv_cnn_forward")
        return (logits, digits, conf) if want_digits else logits

    def _cnn3_forward(self, entry, nfeat, x, want_digits, want_features, glue):
        """cnn3_forward through the library's `entry`_f32 / `entry`_cells_u8, for a model with `nfeat` pooled features."""
        x, logits, digits, conf = self._cnn_args(x, want_digits)
        B = x.shape[0]
        if want_features and x.dtype == torch.uint8:
            raise ValueError(f"want_features needs f32 input ({entry}_f32)")
        feats = torch.empty((B, nfeat), dtype=torch.float32, device=self.device) if want_features else None
        if x.dtype == torch.uint8:
            rc = getattr(self._lib, entry + "_cells_u8")(self._h, _ptr(x), B, int(glue), _ptr(logits), _opt_ptr(digits), _opt_ptr(conf), _stream_ptr())
        else:
            rc = getattr(self._lib, entry + "_f32")(self._h, _ptr(x), B, _ptr(logits), _opt_ptr(feats), _opt_ptr(digits), _opt_ptr(conf), _stream_ptr())
        self._check(rc, entry)
        out = (logits, digits, conf) if want_digits else (logits,)
        if want_features:
            out += (feats,)
        return out if len(out) > 1 else logits

    def cnn3_forward(self, x, want_digits=False, want_features=False, glue=0):
        """DigitCNNv3.forward (ml/model_v3.py): x f32 [B,1,28,28], or u8 [B,28,28] cells with the run_v2.py glue fused in (as cnn_forward)
        -> logits [B,10]; with want_digits (logits, digits, conf), conf = softmax(logits / temperature)[digit]; with want_features the
        128 pooled features [B,128] come last (f32 input only)."""
        return self._cnn3_forward("sv_cnn3_forward", 128, x, want_digits, want_features, glue)

    def cnn3_forward_mc(self, x, n_samples, p_spatial, p_fc, seed, offset, masks=None, want_logits=False, want_masks=False):
        """MC dropout, DigitCNNv3.forward_with_uncertainty (ml/model_v3.py:186-214) with BatchNorm on its running statistics
        (sv_cnn3_forward_mc_f32 has the semantics): x f32 [B,1,28,28] -> (mean_probs f32 [B,10], std_probs f32 [B,10], predicted int64 [B]);
        with want_logits the per-sample logits f32 [S,B,10] follow, with want_masks the keep masks that were used, a tuple of u8 [S,B,32],
        [S,B,64], [S,B,128].  masks: such a tuple to use instead of the generator's draw at (seed, offset), which host.mc_dropout_masks
        restates.  ValueError for n_samples < 1, p_spatial outside [0, 1) or p_fc outside [0, 1].  No host sync."""
        S = int(n_samples)
        if S < 1:
            raise ValueError(f"n_samples must be at least 1, got {n_samples}")
        if not 0.0 <= float(p_spatial) < 1.0:
            raise ValueError(f"spatial dropout rate must be in [0, 1), got {p_spatial}")
        if not 0.0 <= float(p_fc) <= 1.0:
            raise ValueError(f"dropout rate must be in [0, 1], got {p_fc}")
        x = _dev_tensor(x, "x", torch.float32, self.device, shape=(None, 1, 28, 28)).contiguous()
        B = x.shape[0]
        shapes = ((S, B, 32), (S, B, 64), (S, B, 128))
        if masks is not None:
            if len(masks) != 3:
                raise ValueError("masks: (keep1 [S,B,32], keep3 [S,B,64], keepf [S,B,128])")
            masks = tuple(_dev_tensor(m, "masks", torch.uint8, self.device, shape=sh).contiguous() for m, sh in zip(masks, shapes))
        mean = torch.empty((B, 10), dtype=torch.float32, device=self.device)
        std = torch.empty((B, 10), dtype=torch.float32, device=self.device)
        pred = torch.empty((B,), dtype=torch.int64, device=self.device)
        logits = torch.empty((S, B, 10), dtype=torch.float32, device=self.device) if want_logits else None
        used = tuple(torch.empty(sh, dtype=torch.uint8, device=self.device) for sh in shapes) if want_masks else (None,) * 3
        self._check(self._lib.sv_cnn3_forward_mc_f32(self._h, _ptr(x), B, S, float(p_spatial), float(p_fc), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1),
                                                     *[_opt_ptr(m) for m in (masks or (None,) * 3)], _ptr(mean), _ptr(std), _ptr(pred), _opt_ptr(logits),
                                                     *[_opt_ptr(m) for m in used], _stream_ptr()), "sv_cnn3_forward_mc_f32")
        out = (mean, std, pred)
        if want_logits:
            out += (logits,)
        if want_masks:
            out += (used,)
        return out

    def cnn3_light_forward(self, x, want_digits=False, want_features=False, glue=0):
        """DigitCNNv3Light.forward (ml/model_v3.py), after load_state_dict_v3_light: the arguments and results of cnn3_forward, with 96
        pooled features [B,96]."""
        return self._cnn3_forward("sv_cnn3_light_forward", 96, x, want_digits, want_features, glue)

    def empty_forward(self, x, glue=0):
        """EmptyClassifier.forward (ml/model_v3.py), after load_state_dict_empty: x as cnn3_forward takes it -> logit f32 [B,1]; a cell is
        empty where sigmoid(logit) is below the caller's threshold."""
        x, _, _, _ = self._cnn_args(x, False)
        B = x.shape[0]
        logit = torch.empty((B, 1), dtype=torch.float32, device=self.device)
        if x.dtype == torch.uint8:
            rc = self._lib.sv_empty_forward_cells_u8(self._h, _ptr(x), B, int(glue), _ptr(logit), _stream_ptr())
        else:
            rc = self._lib.sv_empty_forward_f32(self._h, _ptr(x), B, _ptr(logit), _stream_ptr())
        self._check(rc, "sv_empty_forward")
        return logit

    # ---- whole path ---------------------------------------------------------------------------
    def _frames_to_digits(self, entry, frames, minv_dev, out, keep_cells, glue):
        """frames_to_digits through the library's `entry`: sv_frames_to_digits, sv_frames_to_digits_v3 or sv_frames_to_digits_v3_light."""
        frames, pitch, fstride = _frame_layout(frames, self.device)
        n, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
        minv_dev = self._minv(minv_dev, n)
        if out is None:
            out = {"logits": torch.empty((n, 81, 10), dtype=torch.float32, device=self.device),
                   "digits": torch.empty((n, 81), dtype=torch.uint8, device=self.device),
                   "conf": torch.empty((n, 81), dtype=torch.float32, device=self.device)}
            if keep_cells:
                out["cells"] = torch.empty((n, 81, 28, 28), dtype=torch.uint8, device=self.device)
        self._check(getattr(self._lib, entry)(self._h, _ptr(frames), n, H, W, pitch, fstride, _ptr(minv_dev), int(glue), _opt_ptr(out.get("cells")),
                                              _ptr(out["logits"]), _ptr(out["digits"]), _ptr(out["conf"]), _stream_ptr()), entry)
        return out

    def frames_to_digits(self, frames, minv_dev, out=None, keep_cells=False, glue=0):
        """frames u8 [n,H,W,3], minv_dev f64 [n,3,3] on device -> dict(logits [n,81,10], digits [n,81], conf [n,81])."""
        return self._frames_to_digits("sv_frames_to_digits", frames, minv_dev, out, keep_cells, glue)

    def frames_to_digits_v3(self, frames, minv_dev, out=None, keep_cells=False, glue=0):
        """frames_to_digits with the DigitCNNv3 forward (load_state_dict_v3): same arguments, same dict."""
        return self._frames_to_digits("sv_frames_to_digits_v3", frames, minv_dev, out, keep_cells, glue)

    def frames_to_digits_v3_light(self, frames, minv_dev, out=None, keep_cells=False, glue=0):
        """frames_to_digits with the DigitCNNv3Light forward (load_state_dict_v3_light): same arguments, same dict."""
        return self._frames_to_digits("sv_frames_to_digits_v3_light", frames, minv_dev, out, keep_cells, glue)

    # ---- quality gate (cv/grid_quality.py) ------------------------------------------------------
    def frame_quality_stats(self, frames, out=None):
        """frames u8 [n,H,W,3] (BGR) or [n,H,W] (gray) on device, rows may be padded -> (lap_sum int64 [n], lap_sqsum int64 [n],
        hist int32 [n,256]) on device: the integer sums of cv2.Laplacian(gray, CV_64F) and its square, and calcHist of gray
        (sv_frame_quality_stats_u8).  out: optional tuple of three such tensors to write into."""
        _dev_tensor(frames, "frames", torch.uint8, self.device, ndim=(3, 4))
        ch = 3 if frames.dim() == 4 else 1
        frames, pitch, fstride = _batch_layout(frames, self.device, "frames", ch)
        n, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
        out = out or (None, None, None)
        out = (self._out(out[0], (n,), torch.int64, "lap_sum"), self._out(out[1], (n,), torch.int64, "lap_sqsum"),
               self._out(out[2], (n, 256), torch.int32, "hist"))
        self._check(self._lib.sv_frame_quality_stats_u8(self._h, _ptr(frames), n, H, W, pitch, fstride, ch, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                                        _stream_ptr()), "sv_frame_quality_stats_u8")
        return out

    def grid_line_coverage(self, binary_or_bits, minv_dev, out=None):
        """binary u8 [n,H,W] (any value > 0 is ink) or a bit image int32 [n,H,W//32] (preprocess_bits), minv_dev f64 [n,3,3] from
        corners_to_minv_batch(corners, 450) on device -> counts int32 [n,20] on device: the warped pixels > 0 of compute_completeness's
        bands, band 2i = grid row line i, 2i+1 = grid column line i (sv_grid_line_coverage_u8 / _bits)."""
        x = _dev_tensor(binary_or_bits, "binary_or_bits", (torch.uint8, torch.int32), self.device, ndim=3)
        n, H, W = x.shape
        minv_dev = self._minv(minv_dev, n)
        out = self._out(out, (n, 20), torch.int32, "out")
        if x.dtype == torch.uint8:
            x, pitch, fstride = _plane_layout(x, self.device, "binary_or_bits")
            rc = self._lib.sv_grid_line_coverage_u8(self._h, _ptr(x), n, H, W, pitch, fstride, _ptr(minv_dev), _ptr(out), _stream_ptr())
        else:
            rc = self._lib.sv_grid_line_coverage_bits(self._h, _ptr(x.contiguous()), n, H, W * 32, _ptr(minv_dev), _ptr(out), _stream_ptr())
        self._check(rc, "sv_grid_line_coverage")
        return out

    # ---- validation and correction (resolve/*.py, csrc/k9_resolve.hip) -------------------------------
    _RESOLVE_OUT = (("digits", (81,), torch.uint8), ("conf", (81,), torch.float32), ("index", None, torch.uint8), ("prob", None, torch.float32),
                    ("success", (), torch.uint8), ("num_conflicts_before", (), torch.int32), ("num_conflicts_after", (), torch.int32),
                    ("conflict_count", (81,), torch.uint8), ("n_corrections", (), torch.uint8), ("corr_cells", (3, 3), torch.uint8),
                    ("corr_conf", (3, 2), torch.float32), ("paths_explored", (), torch.int32), ("score", (), torch.float64))

    def resolve_conflicts(self, index, prob, beam_width=5, max_corrections=3, min_alternative_confidence=0.1, acceptance_rule=False, out=None):
        """run_v2's validate_predictions + resolve_conflicts (pipeline/run_v2.py:344-371) for n frames in one launch
        (sv_resolve_conflicts): index u8 [n,81,k], prob f32 [n,81,k] as softmax_topk returns them for n*81 cells -> dict of device
        tensors: digits u8 [n,81], conf f32 [n,81], index u8 [n,81,k], prob f32 [n,81,k] (the resulting cells and their alternatives),
        success u8 [n], num_conflicts_before / num_conflicts_after i32 [n], conflict_count u8 [n,81], n_corrections u8 [n],
        corr_cells u8 [n,3,3] (cell, old digit, new digit), corr_conf f32 [n,3,2] (old, new confidence), paths_explored i32 [n],
        score f64 [n].  Every output equals the reference's; the score equals it to the bit inside this domain: every confidence that
        can enter a path's sum (top-1 of a filled cell, any alternative that passes min_alternative_confidence) is 0 or >= 2^-18, so
        the sum is exact in a double in any order.  softmax_topk's output at the default 0.1 is inside it; lowering
        min_alternative_confidence below 2^-18 leaves it (the score is then within rounding of the reference's, whose own sum()
        depends on the CPython version there).  run_v2 takes the resulting cells when success or num_conflicts_after < num_conflicts_before (:365);
        acceptance_rule=True applies that on the device: a repair run_v2 would not take is dropped and the cell outputs, the conflict
        outputs after and the corrections describe the input.  out: a dict of some of those names -> contiguous tensors to write into;
        only they are computed and returned (None: all of them, newly allocated)."""
        index = _dev_tensor(index, "index", torch.uint8, self.device, shape=(None, 81, None)).contiguous()
        n, _, k = index.shape
        prob = _dev_tensor(prob, "prob", torch.float32, self.device, shape=(n, 81, k)).contiguous()
        shapes = {name: ((n,) + ((81, k) if shape is None else shape), dtype) for name, shape, dtype in self._RESOLVE_OUT}
        if out is None:
            out = {name: torch.empty(shape, dtype=dtype, device=self.device) for name, (shape, dtype) in shapes.items()}
        else:
            unknown = set(out) - set(shapes)
            if unknown:
                raise KeyError(f"not outputs of resolve_conflicts: {sorted(unknown)}")
            for name, t in out.items():
                self._out(t, *shapes[name], name)
        self._check(self._lib.sv_resolve_conflicts(self._h, _ptr(index), _ptr(prob), n, k, int(beam_width), int(max_corrections),
                                                   float(min_alternative_confidence), int(bool(acceptance_rule)),
                                                   *[_opt_ptr(out.get(name)) for name, _, _ in self._RESOLVE_OUT], _stream_ptr()), "sv_resolve_conflicts")
        return out

    # name, per-frame shape, dtype: the order of sv_propagate_constraints' output arguments
    _PROPAGATE_OUT = (("grid", (81,), torch.uint8), ("candidates", (81,), torch.int16), ("is_valid", (), torch.uint8), ("iterations", (), torch.int32),
                      ("contradiction_cell", (), torch.uint8), ("n_resolved", (), torch.uint8), ("resolved", (81, 2), torch.uint8),
                      ("is_fixed", (81,), torch.uint8))

    def propagate_constraints(self, digits, conf=None, max_iterations=100, out=None):
        """run_v2's resolve_with_constraints (pipeline/run_v2.py:373-391, pipeline/constraint_resolver.py:48-267) for n frames in one
        launch (sv_propagate_constraints): digits u8 [n,81] (0 = empty), conf f32 [n,81] or None (1.0 everywhere) -> dict of device
        tensors: grid u8 [n,81], candidates int16 [n,81] (bit d set = d still possible), is_valid u8 [n], iterations i32 [n],
        contradiction_cell u8 [n] (9 * row + col, 255 = none), n_resolved u8 [n], resolved u8 [n,81,2] ((cell, digit) in the reference's
        order, unused entries 255), is_fixed u8 [n,81].  out: a dict of some of those names -> contiguous tensors to write into; only
        they are computed and returned (None: all of them, newly allocated)."""
        digits = _dev_tensor(digits, "digits", torch.uint8, self.device, shape=(None, 81)).contiguous()
        n = digits.shape[0]
        if conf is not None:
            conf = _dev_tensor(conf, "conf", torch.float32, self.device, shape=(n, 81)).contiguous()
        shapes = {name: ((n,) + shape, dtype) for name, shape, dtype in self._PROPAGATE_OUT}
        if out is None:
            out = {name: torch.empty(shape, dtype=dtype, device=self.device) for name, (shape, dtype) in shapes.items()}
        else:
            unknown = set(out) - set(shapes)
            if unknown:
                raise KeyError(f"not outputs of propagate_constraints: {sorted(unknown)}")
            for name, t in out.items():
                self._out(t, *shapes[name], name)
        self._check(self._lib.sv_propagate_constraints(self._h, _ptr(digits), _opt_ptr(conf), n, int(max_iterations),
                                                       *[_opt_ptr(out.get(name)) for name, _, _ in self._PROPAGATE_OUT], _stream_ptr()),
                    "sv_propagate_constraints")
        return out

    # name, per-frame shape, dtype: the order of sv_solve_sudoku_batch's output arguments
    _SOLVE_OUT = (("solution", (81,), torch.uint8), ("result", (), torch.int8), ("nodes", (), torch.int32))
    SOLVE_BUDGET, SOLVE_SKIPPED, SOLVE_MAX_NODES = 2, 3, 65536        # include/sudoku_vision_hip.h

    def solve_sudoku(self, digits, active=None, max_nodes=4096, out=None):
        """run_v2's run_solver (pipeline/run_v2.py:393-407, solver/src/sudoku.c) for n grids in one launch (sv_solve_sudoku_batch, csrc/k14_solve.hip):
        digits u8 [n,81] (0 = empty), active u8 or bool [n] or None (all; a frame with 0 is not solved) -> dict of device tensors:
        solution u8 [n,81] (= digits unless result is 1), result int8 [n] (1 solved, 0 no solution, -1 invalid input, SOLVE_BUDGET: max_nodes
        search nodes were entered and the frame is undecided -- host.solve_sudoku_batch finishes such frames --, SOLVE_SKIPPED: not active),
        nodes int32 [n] (search nodes entered; the root is 1; 0 for results -1 and SOLVE_SKIPPED).  Results, solutions and node counts equal
        host.solve_sudoku_batch's at the same max_nodes, 1..65536.  out: a dict of some of those names -> contiguous tensors to write into;
        only they are returned (None: all of them, newly allocated)."""
        digits = _dev_tensor(digits, "digits", torch.uint8, self.device, shape=(None, 81)).contiguous()
        n = digits.shape[0]
        if active is not None:
            active = _dev_tensor(active, "active", (torch.uint8, torch.bool), self.device, shape=(n,)).contiguous()
        shapes = {name: ((n,) + shape, dtype) for name, shape, dtype in self._SOLVE_OUT}
        if out is None:
            out = {name: torch.empty(shape, dtype=dtype, device=self.device) for name, (shape, dtype) in shapes.items()}
        else:
            unknown = set(out) - set(shapes)
            if unknown:
                raise KeyError(f"not outputs of solve_sudoku: {sorted(unknown)}")
            for name, t in out.items():
                self._out(t, *shapes[name], name)
        self._check(self._lib.sv_solve_sudoku_batch(self._h, _ptr(digits), _opt_ptr(active), n, int(max_nodes),
                                                    *[_opt_ptr(out.get(name)) for name, _, _ in self._SOLVE_OUT], _stream_ptr()), "sv_solve_sudoku_batch")
        return out

    # ---- run_v2's preprocessing (cv/preprocess_v2.py, csrc/k7_preprocess_v2.hip) -------------------
    # Every method takes gray u8 [n,H,W] on device (rows may be padded, frames may have gaps) and returns new dense tensors.
    MORPH_DILATE, MORPH_ERODE, MORPH_CLOSE, MORPH_OPEN = 0, 1, 2, 3
    SHAPE_RECT, SHAPE_ELLIPSE = 0, 1

    def _planes_call(self, entry, x, *args, second=None, image=True, counts=False, name="gray"):
        """The library's entry(ctx, x, n, H, W, pitch, stride, [second,] *args, [image,] [counts,] stream) with x laid out by _plane_layout and
        the outputs allocated here: image u8 [n,H,W], counts int32 [n].  second: (tensor, name) of a second image that the kernels read
        densely: u8, same [n,H,W] as x.  Returns the output, or the tuple of both."""
        x, pitch, fstride = _plane_layout(x, self.device, name)
        n, H, W = x.shape
        if second is not None:
            args = (_ptr(_dev_tensor(second[0], second[1], torch.uint8, self.device, shape=(n, H, W)).contiguous()),) + args
        outs = ([torch.empty((n, H, W), dtype=torch.uint8, device=self.device)] if image else []) + \
               ([torch.empty((n,), dtype=torch.int32, device=self.device)] if counts else [])
        self._check(getattr(self._lib, entry)(self._h, _ptr(x), n, H, W, pitch, fstride, *args, *[_ptr(t) for t in outs], _stream_ptr()), entry)
        return outs[0] if len(outs) == 1 else tuple(outs)

    def morphology(self, gray, op, shape, ksize):
        """cv2.dilate / erode / morphologyEx(CLOSE | OPEN) with getStructuringElement(shape, (ksize, ksize)) (sv_morphology_u8)."""
        return self._planes_call("sv_morphology_u8", gray, int(op), int(shape), int(ksize))

    def box_mean(self, gray, ksize):
        """cv2.blur(gray, (ksize, ksize)) on u8 (sv_box_mean_u8)."""
        return self._planes_call("sv_box_mean_u8", gray, int(ksize))

    def gaussian_blur21(self, gray):
        """cv2.GaussianBlur(gray, (21, 21), 0) on u8 (sv_gaussian_blur21_u8)."""
        return self._planes_call("sv_gaussian_blur21_u8", gray)

    def divide_normalize(self, gray, background):
        """(gray / max(background, 1) * 255) in float32, clipped and truncated to u8 (sv_divide_normalize_u8)."""
        return self._planes_call("sv_divide_normalize_u8", gray, second=(background, "background"))

    def clahe(self, gray, clip_limit=2.0, tiles=(8, 8)):
        """cv2.createCLAHE(clip_limit, tiles).apply(gray), tiles = (tiles_x, tiles_y), any image size (sv_clahe_u8)."""
        return self._planes_call("sv_clahe_u8", gray, float(clip_limit), int(tiles[0]), int(tiles[1]))

    def threshold_sauvola(self, gray, window=25, k=0.2):
        """Sauvola's threshold from exact integer window sums (sv_threshold_sauvola_u8) -> u8 {0,255}."""
        return self._planes_call("sv_threshold_sauvola_u8", gray, int(window), float(k))

    def threshold_count(self, gray, thresh, inv=False):
        """gray > thresh ? 255 : 0 (inv: ? 0 : 255) -> (mask u8 [n,H,W], count int32 [n] of the pixels set), sv_threshold_count_u8."""
        return self._planes_call("sv_threshold_count_u8", gray, int(thresh), int(bool(inv)), counts=True)

    def shadow_mask(self, gray, local_mean, delta=-30):
        """int(gray) - int(local_mean) < delta ? 255 : 0 -> (mask u8 [n,H,W], count int32 [n]), sv_shadow_mask_u8."""
        return self._planes_call("sv_shadow_mask_u8", gray, int(delta), second=(local_mean, "local_mean"), counts=True)

    def count_nonzero(self, img):
        """Pixels != 0 per frame -> int32 [n] (sv_count_nonzero_u8)."""
        return self._planes_call("sv_count_nonzero_u8", img, image=False, counts=True, name="img")


    # ---- grid detection fallbacks (cv/grid_v2.py, csrc/k13_grid_v2.hip) ------------------------------
    def harris_corners(self, gray, max_corners=100, quality_level=0.01, min_distance=10, k=0.04, cand_capacity=None, want_response=False):
        """cv2.goodFeaturesToTrack(gray, max_corners, quality_level, min_distance, blockSize=3, useHarrisDetector=True, k)
        (sv_harris_corners_u8).  gray u8 [H,W] -> corners float32 [m,2] as (x, y); gray u8 [n,H,W] -> (corners float32
        [n,max_corners,2], counts int32 [n]).  A numpy array or a CUDA tensor; a tensor gives tensors.  cand_capacity: room for corner
        candidates per frame; a frame with more raises (SV_ERR_BUFFER), it is never cut short.  None: 2^18, and a frame with more (a noisy
        10-megapixel photo can have them) is run again with room for every pixel, so the default never raises for that.  want_response: also return the Harris
        response float32 [H,W] / [n,H,W] as the last element."""
        d, was_tensor = _to_dev(gray, self)
        single = d.dim() == 2
        x, pitch, fstride = _plane_layout(d[None] if single else d, self.device)
        n, H, W = x.shape
        corners = torch.empty((n, int(max_corners), 2), dtype=torch.float32, device=self.device)
        counts = torch.empty((n,), dtype=torch.int32, device=self.device)
        resp = torch.empty((n, H, W), dtype=torch.float32, device=self.device) if want_response else None
        for cap in ((int(cand_capacity),) if cand_capacity is not None else (min(1 << 18, H * W), min(1 << 24, H * W))):
            rc = self._lib.sv_harris_corners_u8(self._h, _ptr(x), n, H, W, pitch, fstride, int(max_corners), float(quality_level), int(min_distance), float(k),
                                                cap, _ptr(corners), _ptr(counts), _opt_ptr(resp), _stream_ptr())
            if rc != -6 or cap >= H * W:                      # SV_ERR_BUFFER: more candidates than `cap`
                break
        self._check(rc, "sv_harris_corners_u8")
        out = (corners[0, :int(counts[0].item())],) if single else (corners, counts)
        if want_response:
            out += (resp[0] if single else resp,)
        out = tuple(_back(t, was_tensor) for t in out)
        return out[0] if len(out) == 1 else out

    # ---- motion gate (cv/stabilizer.py, csrc/k15_motion.hip) -----------------------------------------
    def motion_update(self, frames, prev_small=None, threshold=30.0, dsize=(160, 120), out=None):
        """MotionDetector.update for n consecutive frames of one feed (sv_motion_update_u8).  frames u8 [n,H,W,3] (BGR) or [n,H,W]
        (gray) on device, rows may be padded and frames may have gaps; prev_small u8 [dh,dw] on device: the small image of the frame
        before frames[0], None at the start of a feed; dsize = (dw, dh) as cv2.resize takes it.
        -> (small u8 [n,dh,dw], counts int32 [n]) on device: small[i] = cv2.resize(gray(frames[i]), dsize), counts[i] = pixels with
        |small[i] - small[i-1]| > threshold (counts[0] = 0 without prev_small).  threshold is compared as the reference compares it, a
        Python float against integer differences: d > threshold <=> d > floor(threshold).  out: optional (small, counts) to write
        into; small may not be prev_small.  A wrong dtype, device, rank or prev_small shape is a ValueError."""
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.device != self.device:
            raise ValueError(f"frames must be a uint8 tensor on {self.device}")
        if frames.dim() not in (3, 4) or (frames.dim() == 4 and frames.shape[3] != 3) or 0 in frames.shape:
            raise ValueError(f"frames must have shape [n,H,W,3] or [n,H,W], got {list(frames.shape)}")
        ch = 3 if frames.dim() == 4 else 1
        frames, pitch, fstride = _batch_layout(frames, self.device, "frames", ch)
        n, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
        dw, dh = int(dsize[0]), int(dsize[1])
        if dw < 1 or dh < 1:
            raise ValueError(f"dsize must be positive, got {dsize}")
        if prev_small is not None:
            if not isinstance(prev_small, torch.Tensor) or prev_small.dtype != torch.uint8 or prev_small.device != self.device:
                raise ValueError(f"prev_small must be a uint8 tensor on {self.device}")
            if tuple(prev_small.shape) != (dh, dw):
                raise ValueError(f"prev_small must have shape [{dh},{dw}], got {list(prev_small.shape)}")
            prev_small = prev_small.contiguous()
        t = float(threshold)
        t = 255.0 if not t < 255.0 else (-1.0 if t < 0.0 else float(int(t)))       # floor, exact in the library's float32
        out = out or (None, None)
        small, counts = self._out(out[0], (n, dh, dw), torch.uint8, "small"), self._out(out[1], (n,), torch.int32, "counts")
        self._check(self._lib.sv_motion_update_u8(self._h, _ptr(frames), n, H, W, ch, pitch, fstride, _opt_ptr(prev_small), t, _ptr(small),
                                                  _ptr(counts), dh, dw, _stream_ptr()), "sv_motion_update_u8")
        return small, counts

    # ---- the solution drawn into the frame (resolve/overlay.py, csrc/k16_overlay.hip) ----------------------------------
    def set_overlay_glyphs(self, atlas):
        """atlas uint8 [9,50,50] (host): the coverage glyphs of the digits 1..9 that render_overlay draws (sv_set_overlay_glyphs).  Rows and
        columns 0..2 and 47..49 of every glyph must be zero (NativeError SV_ERR_BAD_ARG otherwise)."""
        a = np.asarray(atlas)
        if a.dtype != np.uint8 or a.shape != (9, 50, 50):
            raise ValueError(f"atlas must be uint8 [9,50,50], got {a.dtype} {list(a.shape)}")
        a = np.ascontiguousarray(a)
        self._check(self._lib.sv_set_overlay_glyphs(self._h, a.ctypes.data_as(C.c_void_p)), "sv_set_overlay_glyphs")
        self._overlay_glyphs = True

    def render_overlay(self, frames, m_dev, digits, classes=None, palette=None, active=None, shadow=True, out=None):
        """Draws 81 digits per frame into BGR frames, in one launch (sv_render_overlay_u8; include/sudoku_vision_hip.h defines every
        pixel).  frames u8 [n,H,W,3] on device (rows may be padded, frames may have gaps: cropped views are read in place); m_dev f64
        [n,3,3] on device, frame -> grid (corners_to_m_batch); digits u8 [n,81], 0 = nothing drawn; classes u8 [n,81] or None (class 0
        everywhere): the row of `palette` a cell is drawn in; palette u8 [k,3] BGR on device or None: (255,100,0) solved, (0,0,0)
        original, (0,0,255) low confidence (pipeline/overlay.py:63-71); a cell with a class >= k is not drawn; active u8 or bool [n] or
        None: frames with 0 come back unchanged; shadow: the drop shadow.  out: None allocates the destination, out=frames draws in
        place, any other u8 [n,H,W,3] tensor (rows may be padded) that does not overlap frames receives the result.  The first call
        sets the default glyphs (overlay_font.default_atlas()) unless set_overlay_glyphs was called."""
        _dev_tensor(frames, "frames", torch.uint8, self.device, shape=(None, None, None, 3))
        in_place = out is frames or (isinstance(out, torch.Tensor) and out.data_ptr() == frames.data_ptr() and out.shape == frames.shape and
                                     out.stride() == frames.stride() and out.dtype == frames.dtype)
        src, pitch, fstride = _frame_layout(frames, self.device)
        if in_place and src is not frames:
            raise ValueError("frames with this layout cannot be drawn in place (rows must be dense in memory)")
        n, H, W = src.shape[0], src.shape[1], src.shape[2]
        if 0 in (n, H, W):
            raise ValueError(f"frames must not be empty, got {list(frames.shape)}")
        m_dev = self._minv(m_dev, n)
        digits = _dev_tensor(digits, "digits", torch.uint8, self.device, shape=(n, 81)).contiguous()
        if classes is not None:
            classes = _dev_tensor(classes, "classes", torch.uint8, self.device, shape=(n, 81)).contiguous()
        k = 3
        if palette is not None:
            palette = _dev_tensor(palette, "palette", torch.uint8, self.device, shape=(None, 3)).contiguous()
            k = palette.shape[0]
            if not 1 <= k <= 256:
                raise ValueError(f"palette must have 1..256 rows, got {k}")
        if active is not None:
            active = _dev_tensor(active, "active", (torch.uint8, torch.bool), self.device, shape=(n,)).contiguous()
        if in_place:
            dst, dpitch, dstride = src, pitch, fstride
        elif out is None:
            dst = torch.empty((n, H, W, 3), dtype=torch.uint8, device=self.device)
            dpitch, dstride = 3 * W, 3 * W * H
        else:
            _dev_tensor(out, "out", torch.uint8, self.device, shape=(n, H, W, 3))
            dst, dpitch, dstride = _frame_layout(out, self.device)
            if dst is not out:
                raise ValueError("out with this layout cannot be written in place (rows must be dense in memory)")
        if not getattr(self, "_overlay_glyphs", False):
            from . import overlay_font
            self.set_overlay_glyphs(overlay_font.default_atlas())
        self._check(self._lib.sv_render_overlay_u8(self._h, _ptr(src), n, H, W, pitch, fstride, _ptr(m_dev), _ptr(digits), _opt_ptr(classes), _opt_ptr(palette), k,
                                                   _opt_ptr(active), int(bool(shadow)), _ptr(dst), dpitch, dstride, _stream_ptr()), "sv_render_overlay_u8")
        return frames if in_place else (dst if out is None else out)

    def warp_affine(self, img, M, dsize, border_value=0):
        """cv2.warpAffine(img, M, dsize=(w, h), INTER_LINEAR, BORDER_CONSTANT, border_value) on gray u8 (sv_warp_affine_u8).  img [H,W] with M
        [2,3], or [n,H,W] with M [n,2,3]: the forward matrices, float64 (numpy or a tensor).  A numpy image or a CUDA tensor; a tensor
        gives a tensor."""
        d, was_tensor = _to_dev(img, self)
        single = d.dim() == 2
        x, pitch, fstride = _plane_layout(d[None] if single else d, self.device, "img")
        n, H, W = x.shape
        m = M if isinstance(M, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(M, np.float64)))
        m = m.to(device=self.device, dtype=torch.float64).contiguous()
        if m.numel() != 6 * n:
            raise ValueError(f"M must hold {n} 2x3 matrices, got shape {list(m.shape)}")
        dw, dh = int(dsize[0]), int(dsize[1])
        out = torch.empty((n, dh, dw), dtype=torch.uint8, device=self.device)
        self._check(self._lib.sv_warp_affine_u8(self._h, _ptr(x), n, H, W, pitch, fstride, _ptr(m), dh, dw, int(border_value), _ptr(out), _stream_ptr()),
                    "sv_warp_affine_u8")
        return _back(out[0] if single else out, was_tensor)

    @staticmethod
    def augment_check_program(steps, n_steps, src_index, n_src, H, W):
        """sv_augment_check_program on a host program: steps [n_out, AUG_MAX_STEPS] of _native.AUG_STEP_DTYPE, n_steps and src_index int32
        [n_out].  Returns the three as contiguous arrays; NativeError (SV_ERR_BAD_ARG, naming the output and the step) for a program the
        kernel would not run as written.  Needs no GPU."""
        steps = np.ascontiguousarray(steps, _native.AUG_STEP_DTYPE)
        n_steps = np.ascontiguousarray(n_steps, np.int32)
        src_index = np.ascontiguousarray(src_index, np.int32)
        n_out = n_steps.shape[0]
        if steps.shape != (n_out, _native.AUG_MAX_STEPS) or src_index.shape != (n_out,):
            raise ValueError(f"steps must be [{n_out},{_native.AUG_MAX_STEPS}] and src_index [{n_out}], got {list(steps.shape)} and {list(src_index.shape)}")
        lib = _native.lib()
        _native.check(lib.sv_augment_check_program(steps.ctypes.data, n_steps.ctypes.data, src_index.ctypes.data, n_out, int(n_src), int(H), int(W)),
                      "sv_augment_check_program", lib)
        return steps, n_steps, src_index

    def augment_upload_program(self, steps, n_steps, src_index, n_src, H, W):
        """A host program, checked (augment_check_program), as the three device tensors `augment` takes: steps as uint8 [n_out, 960]."""
        steps, n_steps, src_index = self.augment_check_program(steps, n_steps, src_index, n_src, H, W)
        raw = torch.from_numpy(steps.view(np.uint8).reshape(steps.shape[0], -1))
        return raw.to(self.device), torch.from_numpy(n_steps).to(self.device), torch.from_numpy(src_index).to(self.device)

    def augment(self, images, steps, n_steps, src_index, seed=0, index_base=0, out=None):
        """K22 (sv_augment_u8): images u8 [n_src,H,W] on the device -> u8 [n_out,H,W], output i = the program steps[i][:n_steps[i]] run on
        images[src_index[i]].  A program given as numpy arrays is checked and uploaded first; one given as device tensors (steps uint8
        [n_out, 960], n_steps and src_index int32 [n_out]: augment_upload_program) is launched as it is -- no host work, so the call can
        be captured in a graph and replayed after the buffers change.  seed and index_base + i key the random fields."""
        x, pitch, fstride = _plane_layout(images, self.device, "images")
        n_src, H, W = x.shape
        if not (4 <= H <= _native.AUG_MAX_SIDE and 4 <= W <= _native.AUG_MAX_SIDE):
            raise ValueError(f"images of {H} x {W}: the augmentation kernel takes sides of 4..{_native.AUG_MAX_SIDE} pixels")
        if not isinstance(steps, torch.Tensor):
            steps, n_steps, src_index = self.augment_upload_program(steps, n_steps, src_index, n_src, H, W)
        n_out = n_steps.shape[0]
        _dev_tensor(steps, "steps", torch.uint8, self.device, shape=(n_out, _native.AUG_MAX_STEPS * _native.AUG_STEP_DTYPE.itemsize))
        _dev_tensor(n_steps, "n_steps", torch.int32, self.device, shape=(n_out,))
        _dev_tensor(src_index, "src_index", torch.int32, self.device, shape=(n_out,))
        if not (steps.is_contiguous() and n_steps.is_contiguous() and src_index.is_contiguous()):
            raise ValueError("the program tensors must be contiguous")
        dst = self._out(out, (n_out, H, W), torch.uint8, "out")
        self._check(self._lib.sv_augment_u8(self._h, _ptr(x), n_src, H, W, pitch, fstride, _ptr(steps), _ptr(n_steps), _ptr(src_index), n_out,
                                            int(seed) & (2 ** 64 - 1), int(index_base), _ptr(dst), _stream_ptr()), "sv_augment_u8")
        return dst

    @staticmethod
    def synth_check_program(cells, steps, n_steps, size, atlas_dims):
        """sv_synth_check_program on a host job: cells [n_out] of _native.SYN_CELL_DTYPE, steps [n_out, AUG_MAX_STEPS] of AUG_STEP_DTYPE, n_steps
        int32 [n_out], atlas_dims int32 [n_slots, 2].  Returns the four as contiguous arrays; NativeError (SV_ERR_BAD_ARG, naming the output
        and the field or step) for a job the kernel would not run as written.  Needs no GPU."""
        cells = np.ascontiguousarray(cells, _native.SYN_CELL_DTYPE)
        steps = np.ascontiguousarray(steps, _native.AUG_STEP_DTYPE)
        n_steps = np.ascontiguousarray(n_steps, np.int32)
        dims = np.ascontiguousarray(atlas_dims, np.int32).reshape(-1, 2)
        n_out = n_steps.shape[0]
        if steps.shape != (n_out, _native.AUG_MAX_STEPS) or cells.shape != (n_out,):
            raise ValueError(f"steps must be [{n_out},{_native.AUG_MAX_STEPS}] and cells [{n_out}], got {list(steps.shape)} and {list(cells.shape)}")
        lib = _native.lib()
        _native.check(lib.sv_synth_check_program(cells.ctypes.data, steps.ctypes.data, n_steps.ctypes.data, n_out, int(size), dims.ctypes.data if len(dims) else None,
                                                 len(dims)), "sv_synth_check_program", lib)
        return cells, steps, n_steps, dims

    @staticmethod
    def synth_atlas(masks):
        """Glyph masks (a list of u8 [h, w] coverage arrays) -> (atlas u8 [n, G, G], dims int32 [n, 2] = (w, h)), G = _native.SYN_GLYPH_SIDE.  A mask
        larger than G on a side is refused."""
        G = _native.SYN_GLYPH_SIDE
        atlas, dims = np.zeros((len(masks), G, G), np.uint8), np.zeros((len(masks), 2), np.int32)
        for k, m in enumerate(masks):
            m = np.asarray(m, np.uint8)
            if m.ndim != 2 or not (1 <= m.shape[0] <= G and 1 <= m.shape[1] <= G):
                raise ValueError(f"glyph mask {k} of shape {list(m.shape)}: the atlas takes masks of 1..{G} pixels on a side")
            atlas[k, :m.shape[0], :m.shape[1]] = m
            dims[k] = (m.shape[1], m.shape[0])
        return atlas, dims

    def synth_upload_program(self, cells, steps, n_steps, size, atlas):
        """A host job, checked (synth_check_program), as the device tensors `synth_cells` takes: cells as uint8 [n_out, 96], steps as uint8
        [n_out, 960], n_steps int32 [n_out], and the atlas pair (u8 [n_slots, G, G], int32 [n_slots, 2])."""
        a, dims = atlas
        a = np.ascontiguousarray(a, np.uint8)
        G = _native.SYN_GLYPH_SIDE
        if a.shape != (len(dims), G, G):
            raise ValueError(f"the atlas must be [{len(dims)},{G},{G}], got {list(a.shape)}")
        cells, steps, n_steps, dims = self.synth_check_program(cells, steps, n_steps, size, dims)
        dev = lambda x: torch.from_numpy(x).to(self.device)
        return (dev(cells.view(np.uint8).reshape(len(cells), -1)), dev(steps.view(np.uint8).reshape(steps.shape[0], -1)), dev(n_steps),
                (dev(a.reshape(len(dims), G, G)), dev(dims)))

    def synth_cells(self, cells, steps, n_steps, size, atlas, seed=0, index_base=0, out=None):
        """K23 (sv_synth_cells_u8): n_out cell records and step programs -> u8 [n_out, size, size] on the device in one launch.  atlas is the
        pair (u8 [n_slots, G, G], int32 [n_slots, 2]) of synth_atlas.  A job given as numpy arrays is checked and uploaded first; one given
        as device tensors (synth_upload_program) is launched as it is -- no host work, so the call can be captured in a graph and replayed
        after the buffers change.  seed and index_base + i key the random fields."""
        size = int(size)
        if not 4 <= size <= _native.AUG_MAX_SIDE:
            raise ValueError(f"cells of {size} x {size}: the generator kernel takes sides of 4..{_native.AUG_MAX_SIDE} pixels")
        if not isinstance(cells, torch.Tensor):
            cells, steps, n_steps, atlas = self.synth_upload_program(cells, steps, n_steps, size, atlas)
        a, dims = atlas
        n_out, n_slots, G = n_steps.shape[0], dims.shape[0], _native.SYN_GLYPH_SIDE
        _dev_tensor(cells, "cells", torch.uint8, self.device, shape=(n_out, _native.SYN_CELL_DTYPE.itemsize))
        _dev_tensor(steps, "steps", torch.uint8, self.device, shape=(n_out, _native.AUG_MAX_STEPS * _native.AUG_STEP_DTYPE.itemsize))
        _dev_tensor(n_steps, "n_steps", torch.int32, self.device, shape=(n_out,))
        _dev_tensor(a, "atlas", torch.uint8, self.device, shape=(n_slots, G, G))
        _dev_tensor(dims, "atlas dims", torch.int32, self.device, shape=(n_slots, 2))
        if not all(t.is_contiguous() for t in (cells, steps, n_steps, a, dims)):
            raise ValueError("the job tensors must be contiguous")
        dst = self._out(out, (n_out, size, size), torch.uint8, "out")
        self._check(self._lib.sv_synth_cells_u8(self._h, _ptr(cells), _ptr(steps), _ptr(n_steps), n_out, size, _ptr(a) if n_slots else None,
                                                _ptr(dims) if n_slots else None, n_slots, int(seed) & (2 ** 64 - 1), int(index_base), _ptr(dst), _stream_ptr()),
                    "sv_synth_cells_u8")
        return dst


_default = {}
_lock = threading.Lock()


def default_context(device=None) -> Context:
    _require_gpu()
    idx = torch.cuda.current_device() if device is None else (torch.device(device).index or 0)
    with _lock:
        if idx not in _default:
            _default[idx] = Context(torch.device("cuda", idx))
        return _default[idx]


def frames_to_digits(frames, corners, state_dict=None, ctx=None):
    """Device-resident hot path: frames u8 [n,H,W,3] (cuda tensor), corners [n,4,2] (host) -> dict of tensors."""
    ctx = ctx or default_context(frames.device)
    if state_dict is not None:
        ctx.load_state_dict(state_dict)
    minv = ctx.minv_to_device(Context.corners_to_minv(corners))
    return ctx.frames_to_digits(frames, minv)
