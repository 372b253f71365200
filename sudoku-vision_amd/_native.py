"""ctypes binding of libsudokuvision_hip.so (include/sudoku_vision_hip.h).  Fails loudly."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libsudokuvision_hip.so")
# test-only superset (csrc/Makefile, include/sudoku_vision_xcheck.h): the product's objects plus independent second implementations
# (csrc/x_cnn_round1.hip, csrc/k1_threshold_mm.hip) for cross-checks.  Loaded by tests/ and tools/ through lib_xcheck(); never by the
# package itself.
XCHECK_LIB_PATH = os.path.join(_HERE, "csrc", "libsudokuvision_xcheck.so")
ABI_VERSION = 2

SV_OK = 0
ERR_NAMES = {-1: "SV_ERR_BAD_ARG", -2: "SV_ERR_HIP", -3: "SV_ERR_NO_WEIGHTS", -4: "SV_ERR_UNSUPPORTED",
             -5: "SV_ERR_DEGENERATE", -6: "SV_ERR_BUFFER"}

_p, _i, _l, _d, _f, _pd = C.c_void_p, C.c_int, C.c_long, C.c_double, C.c_float, C.c_ssize_t

# name -> argtypes; every function returns int unless listed in _RESTYPES
SIGNATURES = {
    "sv_version": [],
    "sv_last_error": [],
    "sv_ctx_create": [_i, C.POINTER(_p)],
    "sv_ctx_destroy": [_p],
    "sv_ctx_reserve": [_p, _l],
    "sv_ctx_set_precision": [_p, _i],
    "sv_load_weights_f32": [_p, _p],
    "sv_timing_begin": [_p],
    "sv_timing_end": [_p, _p, _p, _i],
    "sv_ctx_set_cnn_kernels": [_p, _i],
    "sv_conv_kernel_info": [_p, _p, _p, _p, _p, _p],
    "sv_gray_u8": [_p, _p, _i, _i, _i, _pd, _pd, _p, _p],
    "sv_blur_u8": [_p, _p, _i, _i, _i, _i, _p, _p],
    "sv_adaptive_threshold_u8": [_p, _p, _i, _i, _i, _i, _d, _i, _p, _p],
    "sv_preprocess_u8": [_p, _p, _i, _i, _i, _pd, _pd, _p, _p],
    "sv_solve_sudoku": [_p, _p, _p],
    "sv_solve_sudoku_batch": [_p, _p, _p, _i, _i, _p, _p, _p, _p],
    "sv_solve_sudoku_batch_host": [_p, _p, _i, _i, _p, _p, _p, _i],
    "sv_despeckle_u8": [_p, _p, _i, _i, _i, _p, _p, _p],
    "sv_preprocess_bits_u8": [_p, _p, _i, _i, _i, _pd, _pd, _p, _p],
    "sv_preprocess_warp_cells_u8": [_p, _p, _i, _i, _i, _pd, _pd, _p, _p, _p, _p],
    "sv_despeckle_bits": [_p, _p, _i, _i, _i, _p],
    "sv_component_filter_bits": [_p, _p, _i, _i, _i, _d, _p],
    "sv_component_filter_u8": [_p, _p, _i, _i, _i, _d, _p, _p, _p],
    "sv_copy_to_pinned_host": [_p, _p, _p, C.c_size_t, _p],
    "sv_sparse_bits_record_bytes": [_i, _i, _l],
    "sv_pack_sparse_bits": [_p, _p, _i, _i, _i, _p, _l, _p],
    "sv_find_grid_corners_sparse_batch": [_p, _l, _i, _i, _i, _d, _d, _p, _p, _i],
    "sv_sparse_bits_expand": [_p, _i, _i, _p],
    "sv_host_pool_set_affinity": [_p, _i],
    "sv_find_grid_corners_bits_batch": [_p, _i, _i, _i, _d, _d, _p, _p, _i],
    "sv_corners_to_minv": [_p, _i, _i, _f, _p],
    "sv_corners_to_minv_batch": [_p, _i, _i, _f, _p, _p],
    "sv_find_grid_corners_u8": [_p, _i, _i, _pd, _d, _d, _p],
    "sv_find_grid_corners_batch_u8": [_p, _i, _i, _i, _pd, _pd, _d, _d, _p, _p, _i],
    "sv_find_contours_u8": [_p, _i, _i, _pd, _p, _l, _p, _i, _p, _p],
    "sv_find_contours_bits": [_p, _i, _i, _p, _l, _p, _i, _p, _p],
    "sv_contour_area_i32": [_p, _i, _p],
    "sv_arc_length_i32": [_p, _i, _i, _p],
    "sv_approx_poly_dp_i32": [_p, _i, _d, _i, _p, _p],
    "sv_warp_perspective_u8": [_p, _p, _i, _i, _pd, _i, _p, _i, _p, _p],
    "sv_extract_cells_u8": [_p, _p, _i, _i, _pd, _i, _i, _i, _i, _p, _p],
    "sv_warp_cells_u8": [_p, _p, _i, _i, _i, _pd, _pd, _p, _p, _p],
    "sv_resize_linear_u8": [_p, _p, _i, _i, _pd, _p, _i, _i, _p],
    "sv_cell_ink_ratio_u8": [_p, _p, _l, _i, _p, _p, _p],
    "sv_preprocess_cells_u8": [_p, _p, _l, _p, _p],
    "sv_jpeg_parse": [_p, C.c_size_t, _p],
    "sv_jpeg_entropy_decode": [_p, C.c_size_t, _p, _p, _i],
    "sv_jpeg_entropy_decode_sparse": [_p, C.c_size_t, _p, _p, _p, _l, _p, _p, _i],
    "sv_jpeg_entropy_decode_batch": [_p, _p, _i, _p, _p, _p, _p, _p, _p, _p, _i, _p],
    "sv_jpeg_reconstruct_bgr_u8": [_p, _p, _p, _p, _p, _pd, _p],
    "sv_jpeg_reconstruct_sparse_bgr_u8": [_p, _p, _p, _p, _p, _p, _p, _pd, _p],
    "sv_jpeg_scaled_size": [_p, _i, _p, _p],
    "sv_jpeg_reconstruct_scaled_bgr_u8": [_p, _p, _p, _p, _p, _pd, _p, _i],
    "sv_jpeg_reconstruct_sparse_scaled_bgr_u8": [_p, _p, _p, _p, _p, _p, _p, _pd, _p, _i],
    "sv_jpeg_parse_luma": [_p, C.c_size_t, _p],
    "sv_jpeg_entropy_decode_luma": [_p, C.c_size_t, _p, _p, _i],
    "sv_jpeg_entropy_decode_luma_sparse": [_p, C.c_size_t, _p, _p, _p, _l, _p, _p, _i],
    "sv_jpeg_entropy_decode_luma_batch": [_p, _p, _i, _p, _p, _p, _p, _p, _p, _p, _i, _p],
    "sv_jpeg_reconstruct_gray_u8": [_p, _p, _p, _p, _p, _pd, _p, _i],
    "sv_jpeg_reconstruct_sparse_gray_u8": [_p, _p, _p, _p, _p, _p, _p, _pd, _p, _i],
    "sv_jpeg_encode_plan": [_i, _i, _i, _i, _i, _i, _p],
    "sv_jpeg_encode_bound": [_p, _l],
    "sv_jpeg_forward_bgr_u8": [_p, _p, _p, _i, _pd, _pd, _p, _p, _p, _p, _p, _p],
    "sv_jpeg_forward_gray_u8": [_p, _p, _p, _i, _pd, _pd, _p, _p, _p, _p, _p, _p],
    "sv_jpeg_entropy_encode": [_p, _p, _p, _p, _l, _p, C.c_size_t, _p, _i],
    "sv_jpeg_entropy_encode_batch": [_p, _i, _p, _p, _p, _p, _p, _p, _p, _i, _p],
    "sv_png_encode_plan": [_i, _i, _i, _i, _i, _i, _p],
    "sv_png_deflate_bgr_u8": [_p, _p, _p, _i, _pd, _pd, _p, _p, _p, _p, _p],
    "sv_png_deflate_gray_u8": [_p, _p, _p, _i, _pd, _pd, _p, _p, _p, _p, _p],
    "sv_png_assemble": [_p, _p, _p, _p, _p, C.c_size_t, _p],
    "sv_png_assemble_batch": [_p, _i, _p, _p, _p, _p, _p, _p, _i, _p],
    "sv_png_parse": [_p, C.c_size_t, _p],
    "sv_png_inflate": [_p, C.c_size_t, _p, _p, C.c_size_t, _p],
    "sv_png_inflate_batch": [_p, _p, _p, _i, _p, _p, _p, _i, _p],
    "sv_png_reconstruct_bgr_u8": [_p, _p, _p, _p, _p, _i, _p, _pd, _pd, _p, _p],
    "sv_png_reconstruct_gray_u8": [_p, _p, _p, _p, _p, _i, _p, _pd, _pd, _p, _p],
    "sv_dataset_cells": [_p, _p, C.c_size_t, _p, _l, _p, _i, _i, _p, _p, _p, _p],
    "sv_dataset_check_records": [_p, _l, C.c_size_t, _i],
    "sv_softmax_topk_f32": [_p, _p, _l, _i, _p, _p, _p],
    "sv_eval_metrics": [_p, _p, _i, _p, _i, _l, _l, _f, _p, _i, _i] + [_p] * 8 + [_l, _p],
    "sv_eval_metrics_host": [_p, _p, _i, _p, _i, _l, _l, _f, _p, _i, _i] + [_p] * 8 + [_l, _p, _p],
    "sv_resolve_conflicts": [_p, _p, _p, _l, _i, _i, _i, _d, _i] + [_p] * 14,
    "sv_propagate_constraints": [_p, _p, _p, _l, _i] + [_p] * 9,
    "sv_cnn_forward_f32": [_p, _p, _l, _p, _p, _p, _p],
    "sv_cnn_forward_cells_u8": [_p, _p, _l, _i, _p, _p, _p, _p],
    "sv_frames_to_digits": [_p, _p, _i, _i, _i, _pd, _pd, _p, _i, _p, _p, _p, _p, _p],
    "sv_load_weights_v3_f32": [_p, _p, _l, _i],
    "sv_cnn3_forward_f32": [_p, _p, _l, _p, _p, _p, _p, _p],
    "sv_cnn3_forward_cells_u8": [_p, _p, _l, _i, _p, _p, _p, _p],
    "sv_cnn3_forward_mc_f32": [_p, _p, _l, _i, _f, _f, C.c_uint64, C.c_uint64, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p],
    "sv_mc_dropout_masks_host": [C.c_uint64, C.c_uint64, _i, _l, _f, _f, _p, _p, _p],
    "sv_frames_to_digits_v3": [_p, _p, _i, _i, _i, _pd, _pd, _p, _i, _p, _p, _p, _p, _p],
    "sv_load_weights_v3_light_f32": [_p, _p, _l],
    "sv_cnn3_light_forward_f32": [_p, _p, _l, _p, _p, _p, _p, _p],
    "sv_cnn3_light_forward_cells_u8": [_p, _p, _l, _i, _p, _p, _p, _p],
    "sv_frames_to_digits_v3_light": [_p, _p, _i, _i, _i, _pd, _pd, _p, _i, _p, _p, _p, _p, _p],
    "sv_load_weights_empty_f32": [_p, _p, _l],
    "sv_empty_forward_f32": [_p, _p, _l, _p, _p],
    "sv_empty_forward_cells_u8": [_p, _p, _l, _i, _p, _p],
    "sv_frame_quality_stats_u8": [_p, _p, _i, _i, _i, _pd, _pd, _i, _p, _p, _p, _p],
    "sv_grid_line_coverage_u8": [_p, _p, _i, _i, _i, _pd, _pd, _p, _p, _p],
    "sv_grid_line_coverage_bits": [_p, _p, _i, _i, _i, _p, _p, _p],
    "sv_morphology_u8": [_p, _p, _i, _i, _i, _pd, _pd, _i, _i, _i, _p, _p],
    "sv_box_mean_u8": [_p, _p, _i, _i, _i, _pd, _pd, _i, _p, _p],
    "sv_gaussian_blur21_u8": [_p, _p, _i, _i, _i, _pd, _pd, _p, _p],
    "sv_divide_normalize_u8": [_p, _p, _i, _i, _i, _pd, _pd, _p, _p, _p],
    "sv_clahe_u8": [_p, _p, _i, _i, _i, _pd, _pd, _d, _i, _i, _p, _p],
    "sv_threshold_sauvola_u8": [_p, _p, _i, _i, _i, _pd, _pd, _i, _d, _p, _p],
    "sv_threshold_count_u8": [_p, _p, _i, _i, _i, _pd, _pd, _i, _i, _p, _p, _p],
    "sv_shadow_mask_u8": [_p, _p, _i, _i, _i, _pd, _pd, _p, _i, _p, _p, _p],
    "sv_count_nonzero_u8": [_p, _p, _i, _i, _i, _pd, _pd, _p, _p],
    "sv_harris_corners_u8": [_p, _p, _i, _i, _i, _pd, _pd, _i, _d, _i, _d, _i, _p, _p, _p, _p],
    "sv_warp_affine_u8": [_p, _p, _i, _i, _i, _pd, _pd, _p, _i, _i, _i, _p, _p],
    "sv_find_grid_corners_v2_u8": [_p, _i, _i, _pd, _d, _d, _p],
    "sv_find_grid_corners_v2_batch_u8": [_p, _i, _i, _i, _pd, _pd, _d, _d, _p, _p, _i],
    "sv_hough_lines_p_u8": [_p, _i, _i, _pd, _d, _d, _i, _i, _i, _p, _i, _p],
    "sv_motion_update_u8": [_p, _p, _i, _i, _i, _i, _pd, _pd, _p, _f, _p, _p, _i, _i, _p],
    "sv_corners_to_m_batch": [_p, _i, _i, _f, _p, _p],
    "sv_set_overlay_glyphs": [_p, _p],
    "sv_augment_u8": [_p, _p, _i, _i, _i, _pd, _pd, _p, _p, _p, _l, C.c_uint64, _l, _p, _p],
    "sv_augment_check_program": [_p, _p, _p, _l, _i, _i, _i],
    "sv_augment_rotation_matrix": [_d, _d, _d, _d, _p],
    "sv_augment_perspective_matrix": [_p, _p, _p],
    "sv_augment_elastic_taps": [_d, _p, _i, _p],
    "sv_augment_field_host": [C.c_uint64, _l, _i, C.c_uint32, _i, _i, _p],
    "sv_synth_cells_u8": [_p, _p, _p, _p, _l, _i, _p, _p, _i, C.c_uint64, _l, _p, _p],
    "sv_synth_check_program": [_p, _p, _p, _l, _i, _p, _i],
    "sv_synth_gaussian_taps_q8": [_i, _d, _p],
    "sv_render_overlay_u8": [_p, _p, _i, _i, _i, _pd, _pd, _p, _p, _p, _p, _i, _p, _i, _p, _pd, _pd, _p],
}
_RESTYPES = {"sv_last_error": C.c_char_p, "sv_sparse_bits_record_bytes": C.c_long, "sv_jpeg_encode_bound": C.c_long}
# what libsudokuvision_xcheck.so exports on top of SIGNATURES (include/sudoku_vision_xcheck.h)
XCHECK_SIGNATURES = {
    "sv_preprocess_stats": [_p, _p, _p],
    "sv_preprocess_mm_u8": [_p, _p, _i, _i, _i, _pd, _pd, _p, _p, _p],
    "svx_ctx_set_fc_frame_kernel": [_p, _i],
    "svx_ctx_set_motion_shape": [_p, _i],
}



class JpegInfo(C.Structure):
    """sv_jpeg_info of include/sudoku_vision_hip.h"""
    _fields_ = [(n, C.c_int) for n in ("width", "height", "out_width", "out_height", "components", "h_samp", "v_samp",
                                        "orientation", "restart_interval")] + [("coef_count", C.c_long), ("sparse_capacity", C.c_long)]

class JpegEnc(C.Structure):
    """sv_jpeg_enc of include/sudoku_vision_hip.h"""
    _fields_ = [("info", JpegInfo), ("quality", C.c_int), ("quant", C.c_uint16 * 192), ("recip", C.c_uint32 * 192), ("out_bound", C.c_long)]

class PngEnc(C.Structure):
    """sv_png_enc of include/sudoku_vision_hip.h"""
    _fields_ = [(n, C.c_int) for n in ("width", "height", "channels", "filter", "strategy", "band_rows", "bands")] + \
               [(n, C.c_long) for n in ("row_bytes", "filtered_bytes", "slot_bytes", "stream_bound", "out_bound")]

class PngInfo(C.Structure):
    """sv_png_info of include/sudoku_vision_hip.h"""
    _fields_ = [(n, C.c_int) for n in ("width", "height", "bit_depth", "color_type", "interlace", "channels", "bpp", "palette_entries")] + \
               [(n, C.c_long) for n in ("row_bytes", "filtered_bytes", "idat_offset")] + [("palette", C.c_uint8 * 768)]

EVAL_MAX_BINS = 64

class EvalStats(C.Structure):
    """sv_eval_stats of include/sudoku_vision_hip.h"""
    _fields_ = [("confusion", (C.c_uint64 * 10) * 10)] + [(n, C.c_uint64) for n in ("n", "n_correct", "n_wrong", "bad_labels", "nonfinite")] + \
               [(n, C.c_uint64 * EVAL_MAX_BINS) for n in ("bin_count", "bin_correct", "bin_conf")] + \
               [(n, C.c_uint64 * 3) for n in ("tot_count", "tot_correct", "tot_conf")]

# sv_eval_failure of include/sudoku_vision_hip.h, as a numpy record of 48 bytes
EVAL_FAILURE_DTYPE = np.dtype([("index", "<i8"), ("label", "<i4"), ("pred", "<i4"), ("conf", "<f4"), ("true_prob", "<f4"), ("top3_index", "<i4", (3,)),
                               ("top3_prob", "<f4", (3,))])

# sv_aug_step of include/sudoku_vision_hip.h as a numpy record of 96 bytes: d and f name the same 72 bytes
AUG_MAX_STEPS, AUG_MAX_SIDE, AUG_MAX_RADIUS = 10, 64, 16
AUG_STEP_DTYPE = np.dtype({"names": ["op", "i", "d", "f"], "formats": ["<i4", ("<i4", (5,)), ("<f8", (9,)), ("<f4", (18,))], "offsets": [0, 4, 24, 24],
                           "itemsize": 96})
# sv_syn_cell of include/sudoku_vision_hip.h as a numpy record of 96 bytes, and K23's kinds and ops
SYN_GLYPH_SIDE, SYN_BG_SLOT = 32, 255
SYN_CELL_DTYPE = np.dtype([("bg_kind", "<i4"), ("bg_value", "<i4"), ("bg_salt", "<i4"), ("grad_dir", "<i4"), ("grain_stride", "<i4"), ("grain_d", "<u4", (2,)),
                           ("art_edges", "<i4"), ("art_width", "<i4"), ("art_dark", "<i4"), ("smudge", "<i4", (4,)), ("glyph_slot", "<i4"), ("glyph_x", "<i4"),
                           ("glyph_y", "<i4"), ("glyph_ink", "<i4"), ("bg_d", "<f8", (3,))])
SYN_BG_PLAIN, SYN_BG_TEXTURED, SYN_BG_GRADIENT, SYN_BG_NOISY, SYN_BG_KEEP = range(5)
SYN_AFFINE_CONST, SYN_PERSPECTIVE_CONST, SYN_SCALE_PAD, SYN_GAUSS_BLUR, SYN_ERODE, SYN_DILATE = range(32, 38)
AUG_NONE, AUG_AFFINE, AUG_PERSPECTIVE, AUG_BRIGHTNESS, AUG_CONTRAST, AUG_BLUR, AUG_SCALE, AUG_FILL_RECT, AUG_ELASTIC, AUG_NOISE_GAUSS, AUG_NOISE_SP = range(11)

PNG_PALETTE_STRIDE = 1024
# sv_dataset_record of include/sudoku_vision_hip.h as a numpy record of 16 bytes, and K24's modes, limits and status bits
DATASET_RECORD_DTYPE = np.dtype([("offset", "<u8"), ("width", "<u2"), ("height", "<u2"), ("color_type", "u1"), ("bit_depth", "u1"), ("palette", "<u2")])
CELLS_GRAY, CELLS_DATASET = 0, 1
CELLS_MAX_SIDE, CELLS_NO_PALETTE = 64, 0xffff
CELLS_STATUS_PALETTE, CELLS_STATUS_REFUSED = 1, 2


_lib = None
_xlib = None


class NativeError(RuntimeError):
    pass


def lib():
    """Loads the HIP library once.  torch is imported first so that the process holds a single HIP
    runtime (torch's libamdhip64 and the one this library links share a soname)."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"or `make -C sudoku-vision_amd/csrc`.  There is no CPU fallback.")
        _lib = _bind(C.CDLL(LIB_PATH), SIGNATURES)
    return _lib


def _bind(handle, signatures):
    for name, args in signatures.items():
        fn = getattr(handle, name)  # AttributeError = ABI mismatch, let it surface
        fn.argtypes = args
        fn.restype = _RESTYPES.get(name, C.c_int)
    v = handle.sv_version()
    if v != ABI_VERSION:
        raise NativeError(f"{getattr(handle, '_name', 'library')}: ABI version {v}, this package binds version {ABI_VERSION}: rebuild (make -C sudoku-vision_amd/csrc)")
    return handle


def lib_xcheck():
    """The test-only superset library (cross-check kernels).  For tests/ and tools/ only."""
    global _xlib
    if _xlib is None:
        import torch  # noqa: F401
        if not os.path.exists(XCHECK_LIB_PATH):
            raise NativeError(f"{XCHECK_LIB_PATH} is missing: make -C sudoku-vision_amd/csrc libsudokuvision_xcheck.so")
        _xlib = _bind(C.CDLL(XCHECK_LIB_PATH), {**SIGNATURES, **XCHECK_SIGNATURES})
    return _xlib


def check(rc: int, what: str = "", handle=None):
    if rc != SV_OK:
        msg = (handle or lib()).sv_last_error().decode("utf-8", "replace")
        raise NativeError(f"{what or 'libsudokuvision_hip'}: {ERR_NAMES.get(rc, rc)}: {msg}")
