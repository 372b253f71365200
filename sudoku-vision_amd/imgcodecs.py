"""MI355X counterpart of the one cv2.imgcodecs call on the path: `cv2.imread(path)` (pipeline/run.py:250,
pipeline/run_v2.py:267, tests/test_integration.py:126) for JPEG files -- same return convention: a BGR uint8 numpy array,
or None when the file cannot be read or is not a decodable image (cv2.imread does not raise).  JPEG flavours this build
does not decode (progressive, arithmetic, CMYK, 12-bit) raise NativeError instead of returning a wrong image.

`cv2.imread(path, cv2.IMREAD_REDUCED_COLOR_2)` becomes `imread(path, reduce=reduce_from_flags(IMREAD_REDUCED_COLOR_2))`, or
`imread(path, reduce=2)`: libjpeg's reduced-size decode, bit-identical to cv2's, never reconstructed at full size.
"""
import os

from . import _native
from .runtime import Context, default_context

# cv2's values
IMREAD_COLOR = 1
IMREAD_REDUCED_COLOR_2 = 17
IMREAD_REDUCED_COLOR_4 = 33
IMREAD_REDUCED_COLOR_8 = 65
_REDUCE_OF_FLAGS = {IMREAD_COLOR: 1, IMREAD_REDUCED_COLOR_2: 2, IMREAD_REDUCED_COLOR_4: 4, IMREAD_REDUCED_COLOR_8: 8}


def reduce_from_flags(flags):
    """cv2.imread's flags argument -> reduce=.  Only the colour reads this front end performs: IMREAD_COLOR and IMREAD_REDUCED_COLOR_*."""
    try:
        return _REDUCE_OF_FLAGS[flags]
    except (KeyError, TypeError):
        raise ValueError(f"imread flags {flags!r}: only IMREAD_COLOR and IMREAD_REDUCED_COLOR_2/4/8 are decoded here") from None


def imdecode(buf, device=False, ctx=None, threads=1, reduce=1):
    """bytes of a JPEG file -> BGR image; device=True keeps it on the GPU (CUDA uint8 tensor) for K1/K2.
    reduce = 2, 4 or 8: the image at 1/reduce of its size, ceil(H / reduce) x ceil(W / reduce)."""
    reduce = Context.jpeg_reduce_arg(reduce)
    data = bytes(buf)
    ctx = ctx or default_context()
    try:
        img = ctx.imdecode(data, threads=threads, reduce=reduce)
    except _native.NativeError as e:
        if "SV_ERR_UNSUPPORTED" in str(e):
            raise
        return None
    return img if device else img.cpu().numpy()


def imread(path, device=False, ctx=None, threads=1, reduce=1):
    reduce = Context.jpeg_reduce_arg(reduce)
    try:
        with open(os.fspath(path), "rb") as f:
            data = f.read()
    except OSError:
        return None
    return imdecode(data, device=device, ctx=ctx, threads=threads, reduce=reduce)
