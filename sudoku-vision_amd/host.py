"""Host (CPU) half of the hot path: the contour-based grid corner search of cv/grid.py:16-71, implemented
in C++ inside libsudokuvision_hip.so (csrc/host_contours.cpp).  Needs no GPU."""
import ctypes as C
import os

import numpy as np

from . import _native


def _bin(binary):
    b = np.asarray(binary)
    if b.dtype != np.uint8 or b.ndim != 2:
        raise TypeError("expected a 2-D uint8 binary image")
    return np.ascontiguousarray(b)


def find_contours(binary):
    """-> list of int32 arrays of shape (N,1,2), in cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) order."""
    b = _bin(binary)
    H, W = b.shape
    lib = _native.lib()
    npts, ncont = C.c_long(), C.c_int()
    rc = lib.sv_find_contours_u8(b.ctypes.data_as(C.c_void_p), H, W, W, None, 0, None, 0, C.byref(npts), C.byref(ncont))
    if rc not in (0, -6):
        _native.check(rc, "sv_find_contours_u8")
    pts = np.empty((max(npts.value, 1), 2), np.int32)
    sizes = np.empty(max(ncont.value, 1), np.int32)
    _native.check(lib.sv_find_contours_u8(b.ctypes.data_as(C.c_void_p), H, W, W, pts.ctypes.data_as(C.c_void_p), npts.value,
                                          sizes.ctypes.data_as(C.c_void_p), ncont.value, C.byref(npts), C.byref(ncont)), "sv_find_contours_u8")
    out, o = [], 0
    for i in range(ncont.value):
        out.append(pts[o:o + sizes[i]].reshape(-1, 1, 2).copy())
        o += sizes[i]
    return out


def find_contours_bits(bits, H, W):
    """bits uint32/int32 [H, W//32] (1 bit per pixel, LSB = leftmost) -> the same list find_contours gives for the unpacked image."""
    b = np.ascontiguousarray(bits).view(np.uint32)
    lib = _native.lib()
    npts, ncont = C.c_long(), C.c_int()
    rc = lib.sv_find_contours_bits(b.ctypes.data_as(C.c_void_p), int(H), int(W), None, 0, None, 0, C.byref(npts), C.byref(ncont))
    if rc not in (0, -6):
        _native.check(rc, "sv_find_contours_bits")
    pts = np.empty((max(npts.value, 1), 2), np.int32)
    sizes = np.empty(max(ncont.value, 1), np.int32)
    _native.check(lib.sv_find_contours_bits(b.ctypes.data_as(C.c_void_p), int(H), int(W), pts.ctypes.data_as(C.c_void_p), npts.value,
                                            sizes.ctypes.data_as(C.c_void_p), ncont.value, C.byref(npts), C.byref(ncont)), "sv_find_contours_bits")
    out, o = [], 0
    for i in range(ncont.value):
        out.append(pts[o:o + sizes[i]].reshape(-1, 1, 2).copy())
        o += sizes[i]
    return out


def _pts(contour):
    return np.ascontiguousarray(np.asarray(contour).reshape(-1, 2), np.int32)


def contour_area(contour) -> float:
    c = _pts(contour)
    v = C.c_double()
    _native.check(_native.lib().sv_contour_area_i32(c.ctypes.data_as(C.c_void_p), c.shape[0], C.byref(v)), "sv_contour_area_i32")
    return v.value


def arc_length(contour, closed=True) -> float:
    c = _pts(contour)
    v = C.c_double()
    _native.check(_native.lib().sv_arc_length_i32(c.ctypes.data_as(C.c_void_p), c.shape[0], int(bool(closed)), C.byref(v)), "sv_arc_length_i32")
    return v.value


def approx_poly_dp(contour, epsilon, closed=True):
    c = _pts(contour)
    out = np.empty((max(c.shape[0], 1), 2), np.int32)
    n = C.c_int()
    _native.check(_native.lib().sv_approx_poly_dp_i32(c.ctypes.data_as(C.c_void_p), c.shape[0], float(epsilon), int(bool(closed)),
                                                      out.ctypes.data_as(C.c_void_p), C.byref(n)), "sv_approx_poly_dp_i32")
    return out[:n.value].reshape(-1, 1, 2).copy()


def find_grid_corners(binary, min_area_ratio=0.1, epsilon_ratio=0.02):
    """-> int32 (4,2) or None."""
    b = _bin(binary)
    H, W = b.shape
    corners = np.empty((4, 2), np.int32)
    rc = _native.lib().sv_find_grid_corners_u8(b.ctypes.data_as(C.c_void_p), H, W, W, float(min_area_ratio), float(epsilon_ratio),
                                               corners.ctypes.data_as(C.c_void_p))
    if rc < 0:
        _native.check(rc, "sv_find_grid_corners_u8")
    return corners if rc == 1 else None


def find_grid_corners_batch(binaries, min_area_ratio=0.1, epsilon_ratio=0.02, threads=None):
    """binaries uint8 [n,H,W] (host) -> (corners int32 [n,4,2], found bool [n])."""
    b = np.asarray(binaries)
    if b.dtype != np.uint8 or b.ndim != 3:
        raise TypeError("expected uint8 [n,H,W]")
    b = np.ascontiguousarray(b)
    n, H, W = b.shape
    corners = np.zeros((n, 4, 2), np.int32)
    found = np.zeros(n, np.uint8)
    threads = threads or min(n, os.cpu_count() or 1)
    _native.check(_native.lib().sv_find_grid_corners_batch_u8(b.ctypes.data_as(C.c_void_p), n, H, W, W, H * W, float(min_area_ratio),
                                                              float(epsilon_ratio), corners.ctypes.data_as(C.c_void_p),
                                                              found.ctypes.data_as(C.c_void_p), int(threads)), "sv_find_grid_corners_batch_u8")
    return corners, found.astype(bool)


def find_grid_corners_v2(binary, min_area_ratio=0.1, epsilon_ratio=0.02):
    """detect_grid_contour's search (cv/grid_v2.py:102-128): as find_grid_corners, but a 4-gon that is not roughly rectangular
    (is_valid_quadrilateral) is passed over for the next contour -> int32 (4,2) or None."""
    b = _bin(binary)
    H, W = b.shape
    corners = np.empty((4, 2), np.int32)
    rc = _native.lib().sv_find_grid_corners_v2_u8(b.ctypes.data_as(C.c_void_p), H, W, W, float(min_area_ratio), float(epsilon_ratio),
                                                  corners.ctypes.data_as(C.c_void_p))
    if rc < 0:
        _native.check(rc, "sv_find_grid_corners_v2_u8")
    return corners if rc == 1 else None


def find_grid_corners_v2_batch(binaries, min_area_ratio=0.1, epsilon_ratio=0.02, threads=None):
    """binaries uint8 [n,H,W] (host) -> (corners int32 [n,4,2], found bool [n]), find_grid_corners_v2 of every image."""
    b = np.asarray(binaries)
    if b.dtype != np.uint8 or b.ndim != 3:
        raise TypeError("expected uint8 [n,H,W]")
    b = np.ascontiguousarray(b)
    n, H, W = b.shape
    corners = np.zeros((n, 4, 2), np.int32)
    found = np.zeros(n, np.uint8)
    threads = threads or min(n, os.cpu_count() or 1)
    _native.check(_native.lib().sv_find_grid_corners_v2_batch_u8(b.ctypes.data_as(C.c_void_p), n, H, W, W, H * W, float(min_area_ratio),
                                                                 float(epsilon_ratio), corners.ctypes.data_as(C.c_void_p),
                                                                 found.ctypes.data_as(C.c_void_p), int(threads)), "sv_find_grid_corners_v2_batch_u8")
    return corners, found.astype(bool)


def hough_lines_p(binary, rho=1.0, theta=np.pi / 180, threshold=100, min_line_length=50, max_line_gap=10):
    """cv2.HoughLinesP(binary, rho, theta, threshold, minLineLength, maxLineGap) -> int32 [N,4] rows (x0, y0, x1, y1) in the order the
    lines are found (N may be 0)."""
    b = _bin(binary)
    H, W = b.shape
    lib = _native.lib()
    cap = 256
    while True:
        lines = np.empty((cap, 4), np.int32)
        count = C.c_int()
        rc = lib.sv_hough_lines_p_u8(b.ctypes.data_as(C.c_void_p), H, W, W, float(rho), float(theta), int(threshold), int(min_line_length),
                                     int(max_line_gap), lines.ctypes.data_as(C.c_void_p), cap, C.byref(count))
        if rc == -6:                                          # SV_ERR_BUFFER: count holds the number of lines
            cap = count.value
            continue
        _native.check(rc, "sv_hough_lines_p_u8")
        return lines[:count.value].copy()


def find_grid_corners_bits_batch(bits, H, W, min_area_ratio=0.1, epsilon_ratio=0.02, threads=None):
    """bits int32/uint32 [n,H,W//32] (host; 1 bit per pixel, LSB = leftmost) -> (corners int32 [n,4,2], found bool [n])."""
    b = np.ascontiguousarray(bits)
    n = b.shape[0]
    corners = np.zeros((n, 4, 2), np.int32)
    found = np.zeros(n, np.uint8)
    threads = threads or min(n, os.cpu_count() or 1)
    _native.check(_native.lib().sv_find_grid_corners_bits_batch(b.ctypes.data_as(C.c_void_p), n, int(H), int(W), float(min_area_ratio), float(epsilon_ratio),
                                                                corners.ctypes.data_as(C.c_void_p), found.ctypes.data_as(C.c_void_p), int(threads)),
                  "sv_find_grid_corners_bits_batch")
    return corners, found.astype(bool)


def set_pool_affinity(cpus):
    """Restrict the library's host worker threads to these CPUs (an iterable of ints; empty = no restriction for new workers)."""
    a = np.ascontiguousarray(sorted(int(c) for c in cpus), np.int32)
    _native.check(_native.lib().sv_host_pool_set_affinity(a.ctypes.data_as(C.c_void_p) if a.size else None, int(a.size)), "sv_host_pool_set_affinity")


def sparse_bits_record_bytes(H, W, cap_values):
    """Bytes of one sparse record (sv_pack_sparse_bits) with room for cap_values non-zero words."""
    r = _native.lib().sv_sparse_bits_record_bytes(int(H), int(W), int(cap_values))
    if r < 0:
        raise ValueError("bad shape for a sparse record (W must be a multiple of 32)")
    return int(r)


def find_grid_corners_sparse_batch(records, H, W, min_area_ratio=0.1, epsilon_ratio=0.02, threads=None):
    """records uint8 [n,stride] (host; Context.pack_sparse_bits' output after the D2H copy) -> (corners int32 [n,4,2], found uint8 [n]);
    found[i] == 2: record i overflowed its capacity and has to be searched from the dense bit image."""
    if records.dtype != np.uint8 or records.ndim != 2 or not records.flags.c_contiguous:
        raise TypeError("records must be a C-contiguous uint8 [n,stride] array")
    n, stride = records.shape
    corners = np.zeros((n, 4, 2), np.int32)
    found = np.zeros(n, np.uint8)
    threads = threads or min(n, os.cpu_count() or 1)
    _native.check(_native.lib().sv_find_grid_corners_sparse_batch(records.ctypes.data_as(C.c_void_p), stride, n, int(H), int(W), float(min_area_ratio),
                                                                  float(epsilon_ratio), corners.ctypes.data_as(C.c_void_p),
                                                                  found.ctypes.data_as(C.c_void_p), int(threads)), "sv_find_grid_corners_sparse_batch")
    return corners, found


def sparse_bits_expand(record, H, W):
    """One sparse record (uint8 [stride], host) -> the dense bit image uint32 [H, W//32]."""
    rec = np.ascontiguousarray(record, np.uint8)
    out = np.empty((H, W // 32), np.uint32)
    _native.check(_native.lib().sv_sparse_bits_expand(rec.ctypes.data_as(C.c_void_p), int(H), int(W), out.ctypes.data_as(C.c_void_p)), "sv_sparse_bits_expand")
    return out


def solve_sudoku(grid):
    """grid: 9x9 (or 81) digits, 0 = empty -> (code, solution 9x9 uint8); code 1 solved, 0 no solution, -1 invalid input
    (the reference solver's SOLVE_* codes).  solution == grid unless solved."""
    g = np.ascontiguousarray(np.asarray(grid).reshape(81))
    if g.min() < 0 or g.max() > 255:
        return -1, np.asarray(grid, np.uint8).reshape(9, 9)
    g = g.astype(np.uint8)
    out = np.empty(81, np.uint8)
    res = C.c_int()
    _native.check(_native.lib().sv_solve_sudoku(g.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(res)), "sv_solve_sudoku")
    return res.value, out.reshape(9, 9)


def solve_sudoku_batch(grids, active=None, max_nodes=0, threads=None):
    """grids uint8 [n,81] or [n,9,9] (host), active [n] or None (all) -> (result int8 [n], solution uint8 [n,9,9], nodes int32 [n]):
    sv_solve_sudoku_batch_host, the host counterpart of Context.solve_sudoku with the same codes (1 solved, 0 no solution, -1 invalid,
    2 the budget of max_nodes search nodes was spent, 3 not active), solutions and node counts.  max_nodes=0: no budget."""
    g = np.asarray(grids)
    if g.dtype != np.uint8 or g.ndim not in (2, 3) or g.shape[1:] not in ((81,), (9, 9)):
        raise TypeError("expected uint8 [n,81] or [n,9,9]")
    g = np.ascontiguousarray(g)
    n = g.shape[0]
    if active is not None:
        active = np.ascontiguousarray(np.asarray(active).reshape(-1) != 0, np.uint8)
        if active.shape != (n,):
            raise ValueError("active must hold one entry per grid")
    if not 0 <= int(max_nodes) < 2 ** 31:
        raise ValueError("max_nodes must be 0 (no budget) or positive")
    result, solution, nodes = np.empty(n, np.int8), np.empty((n, 9, 9), np.uint8), np.empty(n, np.int32)
    threads = threads or max(1, min(n, os.cpu_count() or 1))
    _native.check(_native.lib().sv_solve_sudoku_batch_host(g.ctypes.data_as(C.c_void_p), active.ctypes.data_as(C.c_void_p) if active is not None else None,
                                                           n, int(max_nodes), solution.ctypes.data_as(C.c_void_p), result.ctypes.data_as(C.c_void_p),
                                                           nodes.ctypes.data_as(C.c_void_p), int(threads)), "sv_solve_sudoku_batch_host")
    return result, solution, nodes


# ---- JPEG front end, host half (csrc/host_jpeg.cpp): header parsing and Huffman decoding -------------------
def jpeg_parse(data: bytes):
    """-> _native.JpegInfo (sv_jpeg_info).  Raises NativeError for non-JPEG data and for unsupported JPEG flavours."""
    info = _native.JpegInfo()
    _native.check(_native.lib().sv_jpeg_parse(data, len(data), C.byref(info)), "sv_jpeg_parse")
    return info


def jpeg_entropy_decode(data: bytes, coef=None, quant=None, threads=1):
    """-> (info, coef int16 [coef_count], quant uint16 [3,64]).  coef/quant may be caller-owned (e.g. pinned) numpy arrays."""
    info = jpeg_parse(data)
    if coef is None:
        coef = np.empty(info.coef_count, np.int16)
    if quant is None:
        quant = np.empty((3, 64), np.uint16)
    if coef.dtype != np.int16 or coef.size < info.coef_count or not coef.flags.c_contiguous:
        raise ValueError("coef must be a contiguous int16 array of at least info.coef_count values")
    _native.check(_native.lib().sv_jpeg_entropy_decode(data, len(data), coef.ctypes.data_as(C.c_void_p), quant.ctypes.data_as(C.c_void_p), int(threads)),
                  "sv_jpeg_entropy_decode")
    return info, coef, quant


def jpeg_entropy_decode_sparse(data: bytes, threads=1):
    """-> (info, masks uint64 [blocks], offsets uint32 [blocks], values int16 [used], quant uint16 [3,64]): the compact
    transport form (mask over zigzag positions + first-value index per block, non-zero values in zigzag order)."""
    info = jpeg_parse(data)
    nb = info.coef_count // 64
    masks, offs = np.empty(nb, np.uint64), np.empty(nb, np.uint32)
    vals = np.empty(info.sparse_capacity, np.int16)
    quant = np.empty((3, 64), np.uint16)
    used = C.c_long()
    _native.check(_native.lib().sv_jpeg_entropy_decode_sparse(data, len(data), masks.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p),
                                                              vals.ctypes.data_as(C.c_void_p), vals.size, C.byref(used), quant.ctypes.data_as(C.c_void_p), int(threads)),
                  "sv_jpeg_entropy_decode_sparse")
    return info, masks, offs, vals[:used.value], quant


def jpeg_parse_luma(data: bytes):
    """-> _native.JpegInfo as jpeg_parse, with coef_count and sparse_capacity those of the luma-only decode (Y's blocks alone)."""
    info = _native.JpegInfo()
    _native.check(_native.lib().sv_jpeg_parse_luma(data, len(data), C.byref(info)), "sv_jpeg_parse_luma")
    return info


def jpeg_entropy_decode_luma(data: bytes, threads=1):
    """-> (info, coef int16 [coef_count], quant uint16 [64]): Y's blocks alone, in scan order (MCU after MCU, an MCU's blocks row-major)."""
    info = jpeg_parse_luma(data)
    coef, quant = np.empty(info.coef_count, np.int16), np.empty(64, np.uint16)
    _native.check(_native.lib().sv_jpeg_entropy_decode_luma(data, len(data), coef.ctypes.data_as(C.c_void_p), quant.ctypes.data_as(C.c_void_p), int(threads)),
                  "sv_jpeg_entropy_decode_luma")
    return info, coef, quant


def jpeg_entropy_decode_luma_sparse(data: bytes, threads=1):
    """-> (info, masks uint64 [blocks], offsets uint32 [blocks], values int16 [used], quant uint16 [64]): jpeg_entropy_decode_luma's blocks in
    the compact transport form."""
    info = jpeg_parse_luma(data)
    nb = info.coef_count // 64
    masks, offs = np.empty(nb, np.uint64), np.empty(nb, np.uint32)
    vals = np.empty(info.sparse_capacity, np.int16)
    quant = np.empty(64, np.uint16)
    used = C.c_long()
    _native.check(_native.lib().sv_jpeg_entropy_decode_luma_sparse(data, len(data), masks.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p),
                                                                   vals.ctypes.data_as(C.c_void_p), vals.size, C.byref(used), quant.ctypes.data_as(C.c_void_p),
                                                                   int(threads)), "sv_jpeg_entropy_decode_luma_sparse")
    return info, masks, offs, vals[:used.value], quant


# ---- PNG front end, host half (csrc/host_png.cpp): the container's parser and the inflater ---------------------
def png_parse(data: bytes):
    """-> _native.PngInfo (sv_png_info).  Raises NativeError: SV_ERR_BAD_ARG for anything that is not a well-formed PNG file, SV_ERR_UNSUPPORTED
    for an Adam7 file or one above the size limits."""
    info = _native.PngInfo()
    _native.check(_native.lib().sv_png_parse(data, len(data), C.byref(info)), "sv_png_parse")
    return info


def png_inflate(data: bytes, info=None, filtered=None):
    """-> (info, filtered uint8 [filtered_bytes], row_filter uint8 [height]): the IDAT chunks' zlib stream inflated, and each row's filter byte.
    `filtered` may be a caller-owned (e.g. pinned) contiguous uint8 array; fewer than info.filtered_bytes bytes raise SV_ERR_BUFFER.  Every
    malformed stream raises NativeError (SV_ERR_BAD_ARG)."""
    info = info or png_parse(data)
    if filtered is None:
        filtered = np.empty(info.filtered_bytes, np.uint8)
    if filtered.dtype != np.uint8 or not filtered.flags.c_contiguous:
        raise ValueError("filtered must be a contiguous uint8 array")
    row_filter = np.empty(info.height, np.uint8)
    _native.check(_native.lib().sv_png_inflate(data, len(data), C.byref(info), filtered.ctypes.data_as(C.c_void_p), filtered.size,
                                               row_filter.ctypes.data_as(C.c_void_p)), "sv_png_inflate")
    return info, filtered[:info.filtered_bytes], row_filter


def png_inflate_batch(datas, infos=None, threads=None):
    """-> (infos, [filtered], [row_filter], status int [n]) over `threads` host threads; a file that fails has its sv_status in status[i] (0: fine)
    and nothing is raised for it.  A file sv_png_parse refuses raises."""
    datas = [bytes(d) for d in datas]
    n = len(datas)
    infos = infos or [png_parse(d) for d in datas]
    if len(infos) != n:
        raise ValueError(f"{len(infos)} infos for {n} files")
    arr = (_native.PngInfo * n)(*infos)
    outs = [np.empty(int(i.filtered_bytes), np.uint8) for i in infos]
    rows = [np.empty(int(i.height), np.uint8) for i in infos]
    VP = C.c_void_p * n
    status = (C.c_int * n)()
    if not threads:                                                     # the CPUs this process may run on, 16 at the most: never the whole host
        cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        threads = max(1, min(n, cpus, 16))
    _native.lib().sv_png_inflate_batch((C.c_char_p * n)(*datas), (C.c_size_t * n)(*[len(d) for d in datas]), arr, n, VP(*[o.ctypes.data for o in outs]),
                                       (C.c_size_t * n)(*[o.size for o in outs]), VP(*[r.ctypes.data for r in rows]), int(threads), status)
    return infos, outs, rows, np.array(list(status), np.int32)


# ---- K24's host half: PNG cell files -> the one buffer Context.dataset_cells copies to the device (ml/datasets.py:81, :153: the serial half of
# cv2.imread per sample) -----------
DATASET_TOO_LARGE = 1          # PackedCells.status of a file with a side above 64: not K24's, read it through imdecode_png(gray=True) + resize_linear


class PackedCells:
    """What dataset_pack returns.  `pinned`: one uint8 torch tensor (pinned when a GPU is there) laid out as
    records [n] of _native.DATASET_RECORD_DTYPE at records_at | palettes [n_palettes][1024] at palettes_at | filtered bytes at filtered_at.
    status int32 [n]: 0, a negative sv_status (-1 SV_ERR_BAD_ARG: a file cv2 could not read; -4 SV_ERR_UNSUPPORTED: an Adam7 file) or
    DATASET_TOO_LARGE; such a file's record has sides 0, which the kernel refuses (zeros out, SV_CELLS_STATUS_REFUSED)."""
    __slots__ = ("n", "pinned", "records_at", "palettes_at", "n_palettes", "filtered_at", "filtered_size", "status")

    @property
    def records(self):
        return self.pinned.numpy()[self.records_at:self.records_at + 16 * self.n].view(_native.DATASET_RECORD_DTYPE)


def check_dataset_records(records, filtered_size, n_palettes):
    """sv_dataset_check_records on a numpy array of _native.DATASET_RECORD_DTYPE: raises NativeError naming the first malformed record."""
    records = np.ascontiguousarray(records, _native.DATASET_RECORD_DTYPE)
    _native.check(_native.lib().sv_dataset_check_records(records.ctypes.data_as(C.c_void_p), records.size, int(filtered_size), int(n_palettes)),
                  "sv_dataset_check_records")


def dataset_pack(paths_or_buffers, threads=None):
    """PNG cell files (paths, or bytes-like file contents) -> PackedCells: sv_png_parse per file, sv_png_inflate_batch over `threads` host
    threads (default: the CPUs of this process, 16 at the most) straight into the packed buffer, one record and, for colour type 3, one
    palette per file.  Nothing is raised for a bad file: see PackedCells.status."""
    import torch
    items = list(paths_or_buffers)
    n = len(items)
    if n == 0:
        raise ValueError("dataset_pack needs at least one file")
    status = np.zeros(n, np.int32)
    datas, infos = [None] * n, [None] * n
    for i, it in enumerate(items):
        if isinstance(it, (bytes, bytearray, memoryview)):
            datas[i] = bytes(it)
        else:
            try:
                with open(os.fspath(it), "rb") as f:
                    datas[i] = f.read()
            except OSError:
                status[i] = -1
                continue
        try:
            infos[i] = png_parse(datas[i])
        except _native.NativeError as e:
            status[i] = -4 if "SV_ERR_UNSUPPORTED" in str(e) else -1
            continue
        if max(infos[i].width, infos[i].height) > _native.CELLS_MAX_SIDE:
            status[i] = DATASET_TOO_LARGE
    ok = [i for i in range(n) if status[i] == 0]
    pal_of = {i: k for k, i in enumerate(i for i in ok if infos[i].color_type == 3)}
    sizes = [int(infos[i].filtered_bytes) for i in ok]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    p = PackedCells()
    p.n, p.status, p.n_palettes, p.filtered_size = n, status, len(pal_of), int(offsets[-1])
    p.records_at, p.palettes_at = 0, 16 * n
    p.filtered_at = p.palettes_at + _native.PNG_PALETTE_STRIDE * p.n_palettes
    p.pinned = torch.zeros(p.filtered_at + max(p.filtered_size, 1), dtype=torch.uint8)
    if torch.cuda.is_available():
        p.pinned = p.pinned.pin_memory()
    buf = p.pinned.numpy()
    rec = p.records
    rec["palette"] = _native.CELLS_NO_PALETTE
    for k, i in enumerate(ok):
        inf = infos[i]
        rec[i] = (offsets[k], inf.width, inf.height, inf.color_type, inf.bit_depth, pal_of.get(i, _native.CELLS_NO_PALETTE))
        if i in pal_of:
            at = p.palettes_at + _native.PNG_PALETTE_STRIDE * pal_of[i]
            buf[at:at + 768] = np.frombuffer(bytes(inf.palette), np.uint8)
            buf[at + 768:at + 772] = np.frombuffer(np.uint32(inf.palette_entries).tobytes(), np.uint8)
    m = len(ok)
    if m:
        if not threads:
            cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
            threads = max(1, min(m, cpus, 16))
        base = buf.ctypes.data + p.filtered_at
        VP = C.c_void_p * m
        rcs = (C.c_int * m)()
        _native.lib().sv_png_inflate_batch((C.c_char_p * m)(*[datas[i] for i in ok]), (C.c_size_t * m)(*[len(datas[i]) for i in ok]),
                                           (_native.PngInfo * m)(*[infos[i] for i in ok]), m, VP(*[base + int(o) for o in offsets[:-1]]), (C.c_size_t * m)(*sizes),
                                           None, int(threads), rcs)
        for k, i in enumerate(ok):
            if rcs[k]:
                status[i] = rcs[k]
                rec[i] = (0, 0, 0, 0, 0, _native.CELLS_NO_PALETTE)
    return p


def mc_dropout_masks(seed, offset, n_samples, B, p_spatial=0.1, p_fc=0.5):
    """The keep masks Context.cnn3_forward_mc draws at (seed, offset) when none are passed in (sv_mc_dropout_masks_host; the generator's
    layout is in include/sudoku_vision_hip.h): (keep1 u8 [S,B,32], keep3 [S,B,64], keepf [S,B,128]), 1 = keep.  A cell's sample has the
    same masks whatever B and n_samples are."""
    S, B = int(n_samples), int(B)
    if S < 1 or B < 0:
        raise ValueError(f"n_samples must be at least 1 and B at least 0, got {n_samples}, {B}")
    if not 0.0 <= float(p_spatial) < 1.0:
        raise ValueError(f"spatial dropout rate must be in [0, 1), got {p_spatial}")
    if not 0.0 <= float(p_fc) <= 1.0:
        raise ValueError(f"dropout rate must be in [0, 1], got {p_fc}")
    out = tuple(np.empty((S, B, c), np.uint8) for c in (32, 64, 128))
    _native.check(_native.lib().sv_mc_dropout_masks_host(int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), S, B, float(p_spatial), float(p_fc),
                                                         *[o.ctypes.data_as(C.c_void_p) for o in out]), "sv_mc_dropout_masks_host")
    return out
