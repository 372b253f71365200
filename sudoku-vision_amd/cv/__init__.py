"""Computer-vision half of the hot path; same exports as the reference's cv/__init__.py:8-19.  run_v2's modules
(preprocess_v2, grid_quality) are imported by name, as the reference imports them."""
from .preprocess import grayscale, threshold, blur
from .grid import find_grid_contour, warp_perspective
from .extract import extract_cells
from . import preprocess_v2  # noqa: F401

__all__ = ["grayscale", "threshold", "blur", "find_grid_contour", "warp_perspective", "extract_cells"]
