#!/usr/bin/env python3
"""Generates tests/golden/k1_tie_patches.npz: the seeded searches of tests/threshold_ref.py that take too long to run in every test
session (about 15 s together) -- 15 x 15 gray tie patches (blurred centre mean within 4e-6 of src + 1.5) and 28 x 28 cells whose
CLAHE output has such a pixel at the centre.  tests/test_threshold_ref.py re-runs the first searches and checks every committed
residual."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle")]
import sv_oracle  # noqa: E402
import threshold_ref as T  # noqa: E402

if __name__ == "__main__":
    np.savez_compressed(T.GRAY_PATCH_FILE, gray_patches=T.make_tie_gray_patches(), cells=T.make_tie_cells(sv_oracle.clahe))
    print(T.GRAY_PATCH_FILE)
