// The rules of one K24 record (sv_dataset_record, include/sudoku_vision_hip.h), in one place: the kernel (k24_dataset_cells.hip) applies them to
// every record before it touches a byte, sv_dataset_check_records (sv_api.cpp) reports them on the host, and tools/dev/dataset_records_asan.cpp
// runs them under the sanitizers with a host compiler alone.  Plain functions of their arguments, nothing of HIP.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/sudoku_vision_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SVDS_HD __host__ __device__ inline
#else
#define SVDS_HD inline
#endif

namespace svds {

// What a record's five geometry fields come to
struct Geom {
    int W, H, color_type, bit_depth, channels, bpp, row_bytes;   // row_bytes <= SV_CELLS_MAX_ROW_BYTES
    size_t offset, filtered_bytes;                                // H * (1 + row_bytes) bytes from `offset`
};

// Samples per pixel of a (colour type, depth) pair of the specification, 0 for any other pair
SVDS_HD int channels_of(int color_type, int bit_depth)
{
    const bool d8 = bit_depth == 8, d16 = bit_depth == 16, low = bit_depth == 1 || bit_depth == 2 || bit_depth == 4;
    switch (color_type) {
    case 0: return d8 || d16 || low ? 1 : 0;
    case 2: return d8 || d16 ? 3 : 0;
    case 3: return d8 || low ? 1 : 0;
    case 4: return d8 || d16 ? 2 : 0;
    case 6: return d8 || d16 ? 4 : 0;
    default: return 0;
    }
}

// nullptr and g filled for a record the kernel decodes; else why it is refused (g is then unspecified).  Every field is bounded before it is
// used, so any 16 bytes are a safe argument.
SVDS_HD const char *refuse(const sv_dataset_record &r, size_t filtered_size, int n_palettes, Geom &g)
{
    g.W = r.width; g.H = r.height; g.color_type = r.color_type; g.bit_depth = r.bit_depth;
    if (g.W < 1 || g.W > SV_CELLS_MAX_SIDE || g.H < 1 || g.H > SV_CELLS_MAX_SIDE) return "a side outside 1 .. SV_CELLS_MAX_SIDE";
    g.channels = channels_of(g.color_type, g.bit_depth);
    if (!g.channels) return "a (colour type, bit depth) pair the PNG specification does not have";
    const int bits = g.channels * g.bit_depth;                     // at most 64
    g.bpp = bits >= 8 ? bits / 8 : 1;
    g.row_bytes = (g.W * bits + 7) / 8;                            // at most 64 * 64 / 8 = SV_CELLS_MAX_ROW_BYTES
    g.offset = (size_t)r.offset;
    g.filtered_bytes = (size_t)g.H * (size_t)(1 + g.row_bytes);
    if (r.offset > (uint64_t)filtered_size || g.filtered_bytes > filtered_size - g.offset) return "the filtered stream does not lie inside filtered_size";
    if (g.color_type == 3 && (int)r.palette >= n_palettes) return "colour type 3 without a palette index below n_palettes";
    if (g.color_type != 3 && r.palette != SV_CELLS_NO_PALETTE && (int)r.palette >= n_palettes) return "a palette index at or past n_palettes";
    return nullptr;
}

}  // namespace svds
