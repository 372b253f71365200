"""MI355X counterpart of the one cv2.imgcodecs call on the path: `cv2.imread(path)` (pipeline/run.py:250,
pipeline/run_v2.py:267, tests/test_integration.py:126) for JPEG files -- same return convention: a BGR uint8 numpy array,
or None when the file cannot be read or is not a decodable image (cv2.imread does not raise).  JPEG flavours this build
does not decode (progressive, arithmetic, CMYK, 12-bit) raise NativeError instead of returning a wrong image.

`cv2.imread(path, cv2.IMREAD_REDUCED_COLOR_2)` becomes `imread(path, reduce=reduce_from_flags(IMREAD_REDUCED_COLOR_2))`, or
`imread(path, reduce=2)`: libjpeg's reduced-size decode, bit-identical to cv2's, never reconstructed at full size.

`cv2.imread(path, cv2.IMREAD_GRAYSCALE)` (ml/datasets.py:81, tools/label_cells.py:42 and the other dataset readers) becomes `imread(path, gray=True)`,
or `imread(path, **read_args_from_flags(IMREAD_GRAYSCALE))`: a uint8 [H,W] array, libjpeg's luma-only decode as cv2 performs it, at every `reduce`.

`cv2.imwrite(path, img)` (pipeline/run.py:431) and `cv2.imencode('.jpg', img)` become `imwrite` / `imencode` here, with cv2's signatures and
return conventions: a baseline JPEG, quality 95 and 4:2:0 unless `params` says otherwise, byte for byte the file libjpeg-turbo writes.  The
image may be a numpy array or a CUDA tensor (the frame K16 drew into stays in HBM).  What this encoder does not write -- another extension,
progressive or optimised files -- raises ValueError; nothing falls back to another encoder.

PNG is written under names of its own: `imencode_png(img, params)` and `imwrite_png(path, img, params)` are `cv2.imencode('.png', img, params)` and
`cv2.imwrite('x.png', img, params)`: lossless 8-bit RGB or gray files compressed on the GPU (csrc/k18_png_encode.hip).  `imencode('.png', ...)` and
`imwrite('x.png', ...)` themselves still raise ValueError.

PNG is read under names of its own too: `imdecode_png(buf)` and `imread_png(path)` are `cv2.imdecode(buf, IMREAD_COLOR)` and `cv2.imread(path)` for
PNG files of every colour type and bit depth, non-interlaced: inflate on host threads (csrc/host_png.cpp), unfilter and expansion to BGR on the
GPU (csrc/k19_png_decode.hip); `gray=True` is `IMREAD_GRAYSCALE`, a [H,W] image.  `imread` and `imdecode` themselves still take JPEG only.
"""
import os

import numpy as np

from . import _native
from .runtime import Context, default_context

# cv2's values
IMREAD_COLOR = 1
IMREAD_REDUCED_COLOR_2 = 17
IMREAD_REDUCED_COLOR_4 = 33
IMREAD_REDUCED_COLOR_8 = 65
_REDUCE_OF_FLAGS = {IMREAD_COLOR: 1, IMREAD_REDUCED_COLOR_2: 2, IMREAD_REDUCED_COLOR_4: 4, IMREAD_REDUCED_COLOR_8: 8}
IMREAD_GRAYSCALE = 0
IMREAD_REDUCED_GRAYSCALE_2 = 16
IMREAD_REDUCED_GRAYSCALE_4 = 32
IMREAD_REDUCED_GRAYSCALE_8 = 64
_REDUCE_OF_GRAY_FLAGS = {IMREAD_GRAYSCALE: 1, IMREAD_REDUCED_GRAYSCALE_2: 2, IMREAD_REDUCED_GRAYSCALE_4: 4, IMREAD_REDUCED_GRAYSCALE_8: 8}

# cv2's values
IMWRITE_JPEG_QUALITY = 1
IMWRITE_JPEG_PROGRESSIVE = 2
IMWRITE_JPEG_OPTIMIZE = 3
IMWRITE_JPEG_RST_INTERVAL = 4
IMWRITE_JPEG_SAMPLING_FACTOR = 7
IMWRITE_JPEG_SAMPLING_FACTOR_420 = 0x221111
IMWRITE_JPEG_SAMPLING_FACTOR_422 = 0x211111
IMWRITE_JPEG_SAMPLING_FACTOR_444 = 0x111111
_SAMPLING_OF_FACTOR = {IMWRITE_JPEG_SAMPLING_FACTOR_420: "420", IMWRITE_JPEG_SAMPLING_FACTOR_422: "422", IMWRITE_JPEG_SAMPLING_FACTOR_444: "444"}

# cv2's values
IMWRITE_PNG_COMPRESSION = 16
IMWRITE_PNG_STRATEGY = 17
IMWRITE_PNG_BILEVEL = 18
IMWRITE_PNG_STRATEGY_DEFAULT = 0
IMWRITE_PNG_STRATEGY_FILTERED = 1
IMWRITE_PNG_STRATEGY_HUFFMAN_ONLY = 2
IMWRITE_PNG_STRATEGY_RLE = 3
IMWRITE_PNG_STRATEGY_FIXED = 4


def reduce_from_flags(flags):
    """cv2.imread's flags argument -> reduce=.  Only the colour reads this front end performs: IMREAD_COLOR and IMREAD_REDUCED_COLOR_*."""
    try:
        return _REDUCE_OF_FLAGS[flags]
    except (KeyError, TypeError):
        raise ValueError(f"imread flags {flags!r}: only IMREAD_COLOR and IMREAD_REDUCED_COLOR_2/4/8 are decoded here") from None


def read_args_from_flags(flags):
    """cv2.imread's flags argument -> {"gray": bool, "reduce": int}, the keyword arguments of imread / imdecode here.  The eight reads this front
    end performs: IMREAD_COLOR, IMREAD_GRAYSCALE and their REDUCED_*_2/4/8 forms; anything else (IMREAD_UNCHANGED, _ANYDEPTH, _ANYCOLOR, ...) is a
    ValueError."""
    for gray, table in ((False, _REDUCE_OF_FLAGS), (True, _REDUCE_OF_GRAY_FLAGS)):
        try:
            if not isinstance(flags, bool) and flags in table:
                return {"gray": gray, "reduce": table[flags]}
        except TypeError:
            break
    raise ValueError(f"imread flags {flags!r}: only IMREAD_COLOR, IMREAD_GRAYSCALE and their REDUCED_*_2/4/8 forms are decoded here")


def imdecode(buf, device=False, ctx=None, threads=1, reduce=1, gray=False):
    """bytes of a JPEG file -> BGR image; device=True keeps it on the GPU (CUDA uint8 tensor) for K1/K2.
    reduce = 2, 4 or 8: the image at 1/reduce of its size, ceil(H / reduce) x ceil(W / reduce).
    gray=True: cv2.IMREAD_GRAYSCALE, a [H,W] image decoded from the Y component alone."""
    reduce = Context.jpeg_reduce_arg(reduce)
    data = bytes(buf)
    ctx = ctx or default_context()
    try:
        img = ctx.imdecode(data, threads=threads, reduce=reduce, gray=bool(gray))
    except _native.NativeError as e:
        if "SV_ERR_UNSUPPORTED" in str(e):
            raise
        return None
    return img if device else img.cpu().numpy()


def imread(path, device=False, ctx=None, threads=1, reduce=1, gray=False):
    reduce = Context.jpeg_reduce_arg(reduce)
    try:
        with open(os.fspath(path), "rb") as f:
            data = f.read()
    except OSError:
        return None
    return imdecode(data, device=device, ctx=ctx, threads=threads, reduce=reduce, gray=gray)


def _encode_args(params):
    """cv2's flat [id, value, id, value, ...] list -> Context.imencode's keyword arguments"""
    params = [] if params is None else [int(p) for p in params]
    if len(params) % 2:
        raise ValueError("params is a flat list of (id, value) pairs")
    kw = {"quality": 95, "sampling": "420", "restart": 0}
    for pid, value in zip(params[0::2], params[1::2]):
        if pid == IMWRITE_JPEG_QUALITY:
            kw["quality"] = min(max(value, 0), 100) or 1            # cv2 clamps to 0..100; libjpeg takes 0 as 1
        elif pid == IMWRITE_JPEG_SAMPLING_FACTOR:
            if value not in _SAMPLING_OF_FACTOR:
                raise ValueError(f"IMWRITE_JPEG_SAMPLING_FACTOR {value:#x}: 4:4:4, 4:2:2 and 4:2:0 are written here")
            kw["sampling"] = _SAMPLING_OF_FACTOR[value]
        elif pid == IMWRITE_JPEG_RST_INTERVAL:
            if not 0 <= value <= 65535:
                raise ValueError(f"IMWRITE_JPEG_RST_INTERVAL {value}: 0..65535")
            kw["restart"] = value
        elif pid in (IMWRITE_JPEG_OPTIMIZE, IMWRITE_JPEG_PROGRESSIVE):
            if value:
                raise ValueError("optimised Huffman tables and progressive files are not written here (baseline JPEG with the standard tables only)")
        else:
            raise ValueError(f"imwrite parameter id {pid} is not one this encoder knows")
    return kw


def imencode(ext, img, params=None, ctx=None, threads=1):
    """cv2.imencode: (True, uint8 numpy array [bytes]).  ext: '.jpg' / '.jpeg' / '.jpe'; img: uint8 [H,W,3] BGR or [H,W] gray, numpy or CUDA tensor."""
    import torch
    if str(ext).lower() not in (".jpg", ".jpeg", ".jpe"):
        raise ValueError(f"imencode {ext!r}: only JPEG ('.jpg', '.jpeg', '.jpe') is written here")
    kw = _encode_args(params)
    ctx = ctx or default_context()
    if not isinstance(img, torch.Tensor):
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (1, 3)):
            raise ValueError(f"imencode: expected a uint8 image [H,W], [H,W,1] or [H,W,3], got {img.dtype} {list(img.shape)}")
        if img.ndim == 3 and img.shape[2] == 1:
            img = img[:, :, 0]
        img = torch.from_numpy(np.ascontiguousarray(img)).to(ctx.device)
    data = ctx.imencode(img, threads=threads, **kw)
    return True, np.frombuffer(data, np.uint8)


def imwrite(path, img, params=None, ctx=None, threads=1):
    """cv2.imwrite: True when the file was written, False when it could not be (cv2.imwrite does not raise for that)."""
    ok, data = imencode(os.path.splitext(os.fspath(path))[1], img, params, ctx=ctx, threads=threads)
    try:
        with open(os.fspath(path), "wb") as f:
            f.write(data.tobytes())
    except OSError:
        return False
    return ok


def imdecode_png(buf, device=False, ctx=None, threads=1, *, gray=False):
    """cv2.imdecode(buf, IMREAD_COLOR) for the bytes of a PNG file: a BGR uint8 image [H,W,3] whatever the file's colour type and bit depth (16-bit
    samples keep their high byte, gray is replicated, palettes are looked up, alpha is dropped), or None for a file cv2 would fail to read.
    device=True keeps it on the GPU (CUDA uint8 tensor).  An Adam7 file raises NativeError (SV_ERR_UNSUPPORTED) instead of returning a wrong image.
    gray=True: cv2.imdecode(buf, IMREAD_GRAYSCALE), a uint8 [H,W] image (ml/datasets.py:81, :153): exact for gray files (colour types 0 and 4);
    a colour file gives cv2.cvtColor(cv2.imdecode(buf), COLOR_BGR2GRAY), which is argued, not measured, to be cv2's own gray read: libpng
    converts there and may differ by one level."""
    data = bytes(buf)
    ctx = ctx or default_context()
    try:
        img = ctx.imdecode_png(data, threads=threads, gray=bool(gray))
    except _native.NativeError as e:
        if "SV_ERR_BAD_ARG" not in str(e):                              # only a malformed file is None; a failed launch or allocation is not a bad file
            raise
        return None
    return img if device else img.cpu().numpy()


def imread_png(path, device=False, ctx=None, threads=1, *, gray=False):
    """cv2.imread(path) for a PNG file, whatever the path's extension; None also when the file cannot be opened.  gray=True:
    cv2.imread(path, IMREAD_GRAYSCALE), see imdecode_png."""
    try:
        with open(os.fspath(path), "rb") as f:
            data = f.read()
    except OSError:
        return None
    return imdecode_png(data, device=device, ctx=ctx, threads=threads, gray=gray)


def _png_args(params):
    """cv2's flat [id, value, ...] list -> Context.imencode_png's keyword arguments.  With no parameter cv2 writes the Sub filter on every row,
    Z_BEST_SPEED and Z_RLE, and so does this.  IMWRITE_PNG_COMPRESSION 0: stored blocks only.  1..9: cv2 then leaves libpng's own row filtering
    on, here the adaptive filter (per row the smallest sum of absolute values); the level changes NOTHING else -- this encoder has one effort,
    distance-1 matches and one Huffman code per band, so 1 and 9 write the same bytes."""
    params = [] if params is None else [int(p) for p in params]
    if len(params) % 2:
        raise ValueError("params is a flat list of (id, value) pairs")
    kw = {"filter": "sub", "strategy": "rle"}
    stored = False
    for pid, value in zip(params[0::2], params[1::2]):
        if pid == IMWRITE_PNG_COMPRESSION:
            level = min(max(value, 0), 9)                               # cv2 clamps to 0..9
            stored = level == 0
            if level:
                kw["filter"] = "adaptive"
        elif pid == IMWRITE_PNG_STRATEGY:
            if value == IMWRITE_PNG_STRATEGY_RLE:
                kw["strategy"] = "rle"
            elif value == IMWRITE_PNG_STRATEGY_HUFFMAN_ONLY:
                kw["strategy"] = "huffman_only"
            else:
                raise ValueError(f"IMWRITE_PNG_STRATEGY {value}: IMWRITE_PNG_STRATEGY_RLE and _HUFFMAN_ONLY are written here (matches at distance 1 only)")
        elif pid == IMWRITE_PNG_BILEVEL:
            if value:
                raise ValueError("bi-level PNG files are not written here (8 bits per sample only)")
        else:
            raise ValueError(f"imwrite parameter id {pid} is not one this PNG encoder knows")
    if stored:
        kw["strategy"] = "stored"
    return kw


def imencode_png(img, params=None, ctx=None, threads=1):
    """cv2.imencode('.png', img, params): (True, uint8 numpy array [bytes]).  img: uint8 [H,W,3] BGR, [H,W] or [H,W,1] gray, numpy or CUDA tensor
    (views with dense rows are read in place by their pitch).  params: see _png_args; anything this encoder does not write raises ValueError."""
    import torch
    kw = _png_args(params)
    ctx = ctx or default_context()
    if not isinstance(img, torch.Tensor):
        img = np.asarray(img)
        if img.dtype != np.uint8:
            raise ValueError(f"imencode_png: expected a uint8 image, got {img.dtype}")
        img = torch.from_numpy(np.ascontiguousarray(img)).to(ctx.device)
    if img.dtype != torch.uint8 or img.dim() not in (2, 3) or (img.dim() == 3 and img.shape[2] not in (1, 3)) or img.numel() == 0:
        raise ValueError(f"imencode_png: expected a uint8 image [H,W], [H,W,1] or [H,W,3], got {img.dtype} {list(img.shape)}")
    if img.dim() == 3 and img.shape[2] == 1:
        img = img[:, :, 0]
    data = ctx.imencode_png(img, threads=threads, **kw)
    return True, np.frombuffer(data, np.uint8)


def imwrite_png(path, img, params=None, ctx=None, threads=1):
    """cv2.imwrite(path, img, params) for a PNG file, whatever the path's extension: True when the file was written, False when it could not be."""
    ok, data = imencode_png(img, params, ctx=ctx, threads=threads)
    try:
        with open(os.fspath(path), "wb") as f:
            f.write(data.tobytes())
    except OSError:
        return False
    return ok
