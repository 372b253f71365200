"""The reference's data set chain (ml/datasets.py:18-46, :69-92), restated in numpy from parts that are each pinned elsewhere; nothing of csrc/.

  file -> samples    png_decode_ref: header, zlib.decompress, the unfilter loop
  samples -> gray    cv2.imread(path, IMREAD_GRAYSCALE), written out here: colour types 0 and 4 give the sample itself (16 bits: the high byte;
                     1, 2, 4 bits: x255, x85, x17), alpha dropped; colour types 2, 3, 6 give oracle.gray of png_decode_ref.expand's BGR, i.e.
                     cv2.cvtColor(cv2.imread(path), COLOR_BGR2GRAY); a palette index past PLTE's end gives 0 and ok = False
  resize             oracle.resize_linear to 28 x 28 unless the image is 28 x 28
  preprocess_cell    oracle.preprocess_cells (CLAHE(2.0, (4,4)), adaptiveThreshold(GAUSSIAN_C, BINARY, 11, 2)), then 255 - x
  tensor             np.float32(x) / np.float32(255): one IEEE division, what torch.from_numpy(img).float() / 255.0 computes
"""
import os

import numpy as np

import png_decode_ref as D
import sv_oracle

SCALE = {1: 255, 2: 85, 4: 17}


def gray_of_samples(s, color_type, depth, palette):
    """samples int [H, W, channels] -> (gray u8 [H, W], ok)"""
    if color_type in (0, 4):
        v = s[:, :, 0]
        v = v >> 8 if depth == 16 else v * SCALE[depth] if depth < 8 else v
        return np.ascontiguousarray(v.astype(np.uint8)), True
    bgr, ok = D.expand(s, color_type, depth, palette)
    return sv_oracle.gray(bgr), ok


def gray_decode(data):
    """the bytes of a PNG file -> (gray u8 [H, W], ok)"""
    s, h, _ = D.decode_samples(data)
    return gray_of_samples(s, h["type"], h["depth"], h["palette"])


def cell_of_gray(gray, mode="dataset"):
    """gray u8 [H, W] -> (u8 [28, 28], f32 [28, 28]); mode "gray" stops after the resize"""
    g = np.ascontiguousarray(gray, np.uint8)
    if g.shape != (28, 28):
        g = sv_oracle.resize_linear(g, (28, 28))
    if mode == "dataset":
        g = (255 - sv_oracle.preprocess_cells(g[None])[0]).astype(np.uint8)
    return g, g.astype(np.float32) / np.float32(255)


def cell(data, mode="dataset"):
    """the bytes of a PNG file -> (u8 [28, 28], f32 [28, 28], ok)"""
    gray, ok = gray_decode(data)
    u8, f32 = cell_of_gray(gray, mode)
    return u8, f32, ok


# ---- shared by the CPU and the GPU tests: where the drop-in lives, and the records sv_dataset_check_records and the kernel must refuse ----
ML = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sudoku-vision_amd", "ml")

MALFORMED = {
    "offset past the end": dict(offset=1 << 40),
    "stream past the end": dict(offset=1),
    "a side of 0": dict(width=0),
    "a side of 65": dict(height=65),
    "a bad (type, depth) pair": dict(color_type=2, bit_depth=4),
    "an unknown colour type": dict(color_type=5),
    "a palette index out of range": dict(color_type=3, bit_depth=8, palette=3),
    "colour type 3 without a palette": dict(color_type=3, bit_depth=8),
}


def malformed_records(sva):
    """a valid 28 x 28 gray record, and one copy per entry of MALFORMED with that field changed; filtered_size fits the valid one exactly"""
    base = np.zeros(1, sva._native.DATASET_RECORD_DTYPE)
    base[0] = (0, 28, 28, 0, 8, 0xffff)
    out = {}
    for name, change in MALFORMED.items():
        r = base.copy()
        for k, v in change.items():
            r[k] = v
        out[name] = r
    return base, out, 28 * 29
