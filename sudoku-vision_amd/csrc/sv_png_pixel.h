// The PNG decoder's arithmetic, shared by the device half (k19_png_decode.hip) and the host-side checks (tools/dev/png_decode_asan.cpp): one byte of
// the unfilter (PNG specification, section 9) and one pixel of the expansion to what cv2.imread(path, IMREAD_COLOR) returns.  Plain functions of
// their arguments; which thread calls them, and with whose neighbours, is the kernels' business.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include "sv_device.h"                 // sv_gray_px, for expand_gray (device code only)
#endif

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SVPNG_HD __host__ __device__ inline
#else
#define SVPNG_HD inline
#endif

namespace svpng {

// x: the filtered byte; a, b, c: the unfiltered left, above and above-left bytes (0 where the image has none).  8-bit modular; a filter above 4
// is None.
SVPNG_HD unsigned unfilter_byte(unsigned filter, unsigned x, unsigned a, unsigned b, unsigned c)
{
    unsigned pred = 0;
    if (filter == 1) pred = a;
    else if (filter == 2) pred = b;
    else if (filter == 3) pred = (a + b) >> 1;                         // the 9-bit sum
    else if (filter == 4) {
        const int p = (int)a + (int)b - (int)c;
        const int pa = p > (int)a ? p - (int)a : (int)a - p, pb = p > (int)b ? p - (int)b : (int)b - p, pc = p > (int)c ? p - (int)c : (int)c - p;
        pred = (pa <= pb && pa <= pc) ? a : pb <= pc ? b : c;          // ties: a, then b, then c
    }
    return (x + pred) & 255u;
}

// The geometry the expansion needs
struct Expand {
    int color_type, bit_depth, channels;
};

// One pixel: row = the unfiltered samples of its row, x its column; pal = 256 RGB entries, pal_n how many of them the file has.  Returns
// B | G << 8 | R << 16, bit 24 set for a palette index at or past pal_n (the pixel is then black).
SVPNG_HD uint32_t expand_pixel(const Expand &e, const uint8_t *row, long x, const uint8_t *pal, unsigned pal_n)
{
    unsigned s[3];
    if (e.bit_depth >= 8) {
        const int step = e.bit_depth >> 3;                             // 16-bit samples are big-endian: the first byte is the high one
        const uint8_t *p = row + x * e.channels * step;
        const int colour = (e.color_type == 2 || e.color_type == 6) ? 3 : 1;       // samples before the alpha; an 8-bit palette index is one sample
        for (int k = 0; k < 3; k++) s[k] = p[(k < colour ? k : 0) * step];
    } else {
        const long bit = x * e.bit_depth;
        const unsigned v = ((unsigned)row[bit >> 3] >> (8 - e.bit_depth - (int)(bit & 7))) & ((1u << e.bit_depth) - 1u);     // MSB first
        s[0] = s[1] = s[2] = v;
    }
    if (e.color_type == 3) {
        if (s[0] >= pal_n) return 1u << 24;
        const uint8_t *q = pal + 3 * s[0];
        return (uint32_t)q[2] | (uint32_t)q[1] << 8 | (uint32_t)q[0] << 16;
    }
    if (e.bit_depth < 8) {
        const unsigned scale = e.bit_depth == 1 ? 255u : e.bit_depth == 2 ? 85u : 17u;      // bit replication
        s[0] = s[1] = s[2] = s[0] * scale;
    }
    return (uint32_t)s[2] | (uint32_t)s[1] << 8 | (uint32_t)s[0] << 16;                    // R, G, B in the file -> B, G, R
}

#if defined(__HIPCC__)
// One pixel of the GRAY read, cv2.imread(path, IMREAD_GRAYSCALE) (ml/datasets.py:81, :153; ml/evaluate.py:67): same arguments as expand_pixel,
// one gray byte, bit 8 set for a palette index at or past pal_n (the pixel is then 0).  Colour types 0 and 4: the sample itself (the high byte
// of 16 bits; 1, 2 and 4 bits replicated: x255, x85, x17), alpha dropped.  Colour types 2, 3 and 6: expand_pixel's B, G, R through
// sv_gray_px, K1's BGR -> gray: exactly cv2.cvtColor(cv2.imread(path), COLOR_BGR2GRAY).  cv2's own gray read of a COLOUR file asks libpng for
// the conversion instead, and libpng's rounding is argued, not measured, here: it may differ by one level on colour files.  Gray files, which
// is what every writer of the reference's data sets produces, are exact.  Device only, as sv_gray_px is; its reads are expand_pixel's or fewer, which is what the host-side checks walk.
__device__ inline unsigned expand_gray(const Expand &e, const uint8_t *row, long x, const uint8_t *pal, unsigned pal_n)
{
    if (e.color_type == 0 || e.color_type == 4) {
        if (e.bit_depth >= 8) return row[x * e.channels * (e.bit_depth >> 3)];
        const long bit = x * e.bit_depth;
        const unsigned v = ((unsigned)row[bit >> 3] >> (8 - e.bit_depth - (int)(bit & 7))) & ((1u << e.bit_depth) - 1u);
        return v * (e.bit_depth == 1 ? 255u : e.bit_depth == 2 ? 85u : 17u);
    }
    const uint32_t px = expand_pixel(e, row, x, pal, pal_n);
    if (px >> 24) return 1u << 8;
    return (unsigned)sv_gray_px((int)(px & 255u), (int)(px >> 8 & 255u), (int)(px >> 16 & 255u));
}
#endif

}  // namespace svpng
