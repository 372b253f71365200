// Device half of the JPEG front end (scope row N4; cv2.imread at pipeline/run.py:250): Huffman-decoded coefficient
// blocks -> BGR frame in HBM.  Integer arithmetic throughout, bit-exact with libjpeg's defaults (the decoder behind
// cv2.imread and Pillow): JDCT_ISLOW inverse DCT, "fancy" (triangle-filter) chroma up-sampling, 16-bit fixed-point
// YCbCr -> RGB, EXIF orientation; at full size and at libjpeg's scale_denom 2, 4, 8 (cv2.IMREAD_REDUCED_COLOR_*).
//
// One rule covers every scale (jdmaster.c; jpeg_plan below): at scale 1 / d luma blocks come out at S = 8 / d samples per side, and a
// subsampled component is decoded at a larger block size, up to 8, in place of being up-sampled.  So 4:2:0 chroma is up-sampled at full size
// only (at d > 1 it is decoded at 2S), 4:2:2 chroma keeps its h2v1 step at every d (replication at d = 8, where jdsample.c has no fancy
// filter), and full size is the case where every block size is 8.  The reduced transforms are jidctred.c's 4x4 / 2x2 / 1x1; the image is never
// reconstructed at a larger size than asked for.  One IDCT launch per block size present (at most two), then the colour kernel.  Component
// planes have their own row pitch, a multiple of 4 bytes, and every IDCT thread stores whole 32-bit words:
//   k_jpeg_idct         S = 8: one thread per block row/column, 8 threads per block, 32 blocks per workgroup.  Coefficients come in as one
//                       16-byte load per thread (a block row), are dequantised into LDS, transformed in place column-wise then row-wise
//                       (LDS rows padded to 9 words: both passes conflict-free), and leave as one 8-byte store per thread.
//   k_jpeg_idct4        S = 4: four threads per block, 64 blocks per workgroup.  A thread dequantises block rows t and t + 4 into LDS,
//                       transforms columns t and t + 4, then row t, and stores its 4 samples.  Row and column 4 are never touched.
//   k_jpeg_idct_small   S = 2 or 1: one thread per 4 / S horizontally adjacent blocks, in registers.  S = 2 reads rows and columns
//                       0, 1, 3, 5, 7; S = 1 reads the DC term alone (compact form: mask, offset and at most one value per block).
//   k_jpeg_colour       one thread per OUTPUT pixel (so stores stay coalesced under every orientation): luma sample, the two chroma samples
//                       (same-size plane, or interpolated in closed form: no intermediate full-resolution chroma planes), colour
//                       conversion, 3-byte store.
// The IDCT kernels are HBM-bound, by the coefficient read: 2 B in per full-size sample at every scale, + 1 / d^2 B out.
//
// Stated limit: idct8 (and idct4, idct2 alike) computes in 32-bit int where libjpeg's C code uses long and libjpeg-turbo's SIMD code 16-bit intermediates; the
// three agree while the dequantised coefficients and the first pass's outputs fit 16 bits, which holds for anything an encoder writes
// for 8-bit samples.  Far beyond that they differ and signed overflow here is undefined: such files are outside what this kernel
// promises, and the tests (tests/test_jpeg_crafted.py asserts the bound on its own files) do not feed them.
#include "sv_internal.h"

namespace {

struct JpegIdctGeom {                  // one launch of an IDCT kernel: the components whose blocks come out at the kernel's S
    int bw[3], bh[3];                  // block grid; bh 0 for a component that is not this launch's
    int ipr[3];                        // work items per block row: blocks (S = 8, 4) or groups of 4 / S blocks (S = 2, 1)
    int pitch[3];                      // plane row pitch in bytes, a multiple of 4
    long coef_off[3], plane_off[3];
    long item_start[4];                // prefix sums of work items per component
};

struct JpegColourGeom {                // k_jpeg_colour; W, H: the decoded image as stored, OW, OH: after the EXIF orientation
    int ncomp, W, H, OW, OH, orientation;
    int hup, vup;                      // what is left to up-sample: 1, 1 chroma planes of the image's size; 2, 1 h2v1; 2, 2 h2v2
    int dw, dh;                        // chroma plane size for the fancy filters; dw 0 selects plain replication
    int pitch[3];
    long plane_off[3];
};

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// libjpeg's post-IDCT range-limit table: index (x & 1023), centred on 128
__device__ __forceinline__ unsigned range_limit(int x)
{
    const int v = x & 1023;
    return (unsigned)(v < 128 ? v + 128 : v < 512 ? 255 : v < 896 ? 0 : v - 896);
}

// one 8-point pass of jidctint.c (CONST_BITS 13); the caller applies the pass-specific descale
__device__ __forceinline__ void idct8(const int (&in)[8], int (&out)[8])
{
    int z2 = in[2], z3 = in[6];
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 + z3 * (-15137), tmp3 = z1 + z2 * 6270;
    int tmp0 = (in[0] + in[4]) * 8192, tmp1 = (in[0] - in[4]) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    out[0] = tmp10 + tmp3; out[7] = tmp10 - tmp3;
    out[1] = tmp11 + tmp2; out[6] = tmp11 - tmp2;
    out[2] = tmp12 + tmp1; out[5] = tmp12 - tmp1;
    out[3] = tmp13 + tmp0; out[4] = tmp13 - tmp0;
}

// natural (row-major) position -> zigzag index
__constant__ unsigned char kZigzagOf[64] = {0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
                                            10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// the two 1-D transforms of jidctred.c (CONST_BITS 13); the caller applies the pass-specific descale.  Position 4 is not read.
__device__ __forceinline__ void idct4(const int (&in)[8], int (&out)[4])
{
    const int tmp0 = in[0] * 16384;
    const int tmp2 = in[2] * 15137 + in[6] * (-6270);
    const int tmp10 = tmp0 + tmp2, tmp12 = tmp0 - tmp2;
    const int a = in[7] * (-1730) + in[5] * 11893 + in[3] * (-17799) + in[1] * 8697;
    const int b = in[7] * (-4176) + in[5] * (-4926) + in[3] * 7373 + in[1] * 20995;
    out[0] = tmp10 + b; out[3] = tmp10 - b;
    out[1] = tmp12 + a; out[2] = tmp12 - a;
}

__device__ __forceinline__ void idct2(int i0, int i1, int i3, int i5, int i7, int &o0, int &o1)
{
    const int tmp10 = i0 * 32768;
    const int tmp0 = i7 * (-5906) + i5 * 6967 + i3 * (-10426) + i1 * 29692;
    o0 = tmp10 + tmp0; o1 = tmp10 - tmp0;
}

// One block row, dequantised.  Dense: blk points at the block's 64 values.  SPARSE: the block arrives as (mask over zigzag positions, offset
// of its first value) + the packed value stream, and a coefficient is picked by rank: vals[popcount(mask below the position's zigzag bit)];
// only the columns of COLS are looked up, the others come back 0.  q: the component's quantiser steps.
template <bool SPARSE, unsigned COLS>
__device__ __forceinline__ void deq_row(const short *__restrict__ blk, unsigned long long mask, const short *__restrict__ vals,
                                        const unsigned short *__restrict__ q, int row, int (&out)[8])
{
    const int4 qr = *(const int4 *)(q + row * 8);
    const int qw[4] = {qr.x, qr.y, qr.z, qr.w};
    if (SPARSE) {
        // the conditional load goes into a scalar, not into out[i]: the compiler keeps out[] as one 8-wide value and would carry copies
        // of all of it through every branch (40 more VGPRs)
#pragma unroll
        for (int i = 0; i < 8; i++) {
            int val = 0;
            if ((COLS >> i) & 1) {
                const int z = kZigzagOf[row * 8 + i];
                if ((mask >> z) & 1) val = vals[__popcll(mask & ((1ull << z) - 1))];
            }
            out[i] = val * ((i & 1) ? (int)((unsigned)qw[i >> 1] >> 16) : (int)(qw[i >> 1] & 0xffff));
        }
    } else {
        const int4 raw = *(const int4 *)(blk + row * 8);
        const int cw[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            out[2 * i] = (int)(short)(cw[i] & 0xffff) * (int)(qw[i] & 0xffff);
            out[2 * i + 1] = (cw[i] >> 16) * (int)((unsigned)qw[i] >> 16);
        }
    }
}

__device__ __forceinline__ int component_of(const JpegIdctGeom &g, long item)
{
    return item >= g.item_start[2] ? 2 : item >= g.item_start[1] ? 1 : 0;
}

template <bool SPARSE>
__global__ __launch_bounds__(256) void k_jpeg_idct(const short *__restrict__ coef, const unsigned long long *__restrict__ masks,
                                                    const unsigned *__restrict__ offsets, const short *__restrict__ values,
                                                    const unsigned short *__restrict__ quant, JpegIdctGeom g, u8 *__restrict__ planes)
{
    __shared__ int ws[32][8][9];
    const int tid = threadIdx.x, b = tid >> 3, r = tid & 7;
    const long item = (long)blockIdx.x * 32 + b;
    const bool live = item < g.item_start[3];
    const int c = live ? component_of(g, item) : 0;
    const long lb = item - g.item_start[c];                     // block index within the component
    if (live) {
        const long gb = g.coef_off[c] / 64 + lb;                // block index over all components
        int d[8];
        deq_row<SPARSE, 0xFFu>(SPARSE ? nullptr : coef + gb * 64, SPARSE ? masks[gb] : 0, SPARSE ? values + offsets[gb] : nullptr, quant + c * 64, r, d);
#pragma unroll
        for (int i = 0; i < 8; i++) ws[b][r][i] = d[i];
    }
    __syncthreads();
    int v[8], o[8];
    if (live) {                                                 // pass 1: column r, results scaled up by 2^PASS1_BITS
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = ws[b][i][r];
        idct8(v, o);
#pragma unroll
        for (int i = 0; i < 8; i++) ws[b][i][r] = descale(o[i], 11);
    }
    __syncthreads();
    if (live) {                                                 // pass 2: row r
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = ws[b][r][i];
        idct8(v, o);
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            lo |= range_limit(descale(o[i], 18)) << (8 * i);
            hi |= range_limit(descale(o[4 + i], 18)) << (8 * i);
        }
        const int bx = (int)(lb % g.bw[c]), by = (int)(lb / g.bw[c]);
        *(uint2 *)(planes + g.plane_off[c] + ((long)by * 8 + r) * g.pitch[c] + bx * 8) = make_uint2(lo, hi);
    }
}

template <bool SPARSE>
__global__ __launch_bounds__(256) void k_jpeg_idct4(const short *__restrict__ coef, const unsigned long long *__restrict__ masks,
                                                     const unsigned *__restrict__ offsets, const short *__restrict__ values,
                                                     const unsigned short *__restrict__ quant, JpegIdctGeom g, u8 *__restrict__ planes)
{
    __shared__ int ws[64][73];                                  // [block][row * 9 + column]; 73: neighbouring blocks start 9 banks apart
    const int tid = threadIdx.x, b = tid >> 2, t = tid & 3;
    const long item = (long)blockIdx.x * 64 + b;
    const bool live = item < g.item_start[3];
    const int c = live ? component_of(g, item) : 0;
    const long lb = item - g.item_start[c];                     // block index within the component
    if (live) {
        const long gb = g.coef_off[c] / 64 + lb;                // block index over all components
        const short *blk = SPARSE ? nullptr : coef + gb * 64;
        const unsigned long long mask = SPARSE ? masks[gb] : 0;
        const short *vals = SPARSE ? values + offsets[gb] : nullptr;
#pragma unroll
        for (int h = 0; h < 2; h++) {                           // rows t and t + 4, never row 4
            const int row = t + 4 * h;
            if (row == 4) continue;
            int d[8];
            deq_row<SPARSE, 0xEFu>(blk, mask, vals, quant + c * 64, row, d);
#pragma unroll
            for (int i = 0; i < 8; i++) ws[b][row * 9 + i] = d[i];
        }
    }
    __syncthreads();
    int v[8], o[4];
    v[4] = 0;
    if (live) {                                                 // pass 1: columns t and t + 4, never column 4; in place (a column has one owner)
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int col = t + 4 * h;
            if (col == 4) continue;
#pragma unroll
            for (int i = 0; i < 8; i++) if (i != 4) v[i] = ws[b][i * 9 + col];
            idct4(v, o);
#pragma unroll
            for (int i = 0; i < 4; i++) ws[b][i * 9 + col] = descale(o[i], 12);
        }
    }
    __syncthreads();
    if (live) {                                                 // pass 2: row t
#pragma unroll
        for (int i = 0; i < 8; i++) if (i != 4) v[i] = ws[b][t * 9 + i];
        idct4(v, o);
        unsigned w = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) w |= range_limit(descale(o[i], 19)) << (8 * i);
        const int bx = (int)(lb % g.bw[c]), by = (int)(lb / g.bw[c]);
        *(unsigned *)(planes + g.plane_off[c] + ((long)by * 4 + t) * g.pitch[c] + bx * 4) = w;
    }
}

template <int S, bool SPARSE>
__global__ __launch_bounds__(256) void k_jpeg_idct_small(const short *__restrict__ coef, const unsigned long long *__restrict__ masks,
                                                          const unsigned *__restrict__ offsets, const short *__restrict__ values,
                                                          const unsigned short *__restrict__ quant, JpegIdctGeom g, u8 *__restrict__ planes)
{
    static_assert(S == 1 || S == 2, "block sizes 1 and 2");
    constexpr int G = 4 / S;                                    // blocks per thread: S rows of G * S = 4 samples
    const long item = (long)blockIdx.x * 256 + threadIdx.x;
    if (item >= g.item_start[3]) return;
    const int c = component_of(g, item);
    const long li = item - g.item_start[c];
    const int by = (int)(li / g.ipr[c]), k = (int)(li % g.ipr[c]);
    const unsigned short *q = quant + c * 64;
    unsigned word[S];
#pragma unroll
    for (int i = 0; i < S; i++) word[i] = 0;
#pragma unroll
    for (int j = 0; j < G; j++) {
        const int bx = k * G + j;
        if (bx >= g.bw[c]) break;                               // the pitch is padded to the word: the rest of it stays 0
        const long gb = g.coef_off[c] / 64 + (long)by * g.bw[c] + bx;
        const short *blk = SPARSE ? nullptr : coef + gb * 64;
        const unsigned long long mask = SPARSE ? masks[gb] : 0;
        const short *vals = SPARSE ? values + offsets[gb] : nullptr;
        if (S == 1) {                                           // zigzag position 0 is the DC term: the block's first value when present
            const int dc = SPARSE ? ((mask & 1) ? (int)vals[0] : 0) : (int)blk[0];
            word[0] |= range_limit(descale(dc * (int)q[0], 3)) << (8 * j);
        } else {
            int d[5][8], w0[8], w1[8];
#pragma unroll
            for (int r = 0; r < 5; r++) deq_row<SPARSE, 0xABu>(blk, mask, vals, q, r < 2 ? r : 2 * r - 1, d[r]);    // rows 0, 1, 3, 5, 7
#pragma unroll
            for (int col = 0; col < 8; col++) {
                if (!((0xABu >> col) & 1)) continue;
                int o0, o1;
                idct2(d[0][col], d[1][col], d[2][col], d[3][col], d[4][col], o0, o1);
                w0[col] = descale(o0, 13); w1[col] = descale(o1, 13);
            }
            int o0, o1;
            idct2(w0[0], w0[1], w0[3], w0[5], w0[7], o0, o1);
            word[0] |= (range_limit(descale(o0, 20)) | range_limit(descale(o1, 20)) << 8) << (16 * j);
            idct2(w1[0], w1[1], w1[3], w1[5], w1[7], o0, o1);
            word[S - 1] |= (range_limit(descale(o0, 20)) | range_limit(descale(o1, 20)) << 8) << (16 * j);
        }
    }
#pragma unroll
    for (int i = 0; i < S; i++) *(unsigned *)(planes + g.plane_off[c] + ((long)by * S + i) * g.pitch[c] + 4 * k) = word[i];
}

__device__ __forceinline__ int chroma_sample(const u8 *__restrict__ p, long pw, int dw, int dh, int hmax, int vmax, int x, int y)
{
    if (hmax == 1) return p[(long)y * pw + x];
    const int cx = x >> 1;
    if (vmax == 1) {                                            // h2v1
        const u8 *row = p + (long)y * pw;
        if (dw <= 2) return row[cx];
        const int cur = row[cx];
        if (x & 1) return cx == dw - 1 ? cur : (3 * cur + row[cx + 1] + 2) >> 2;
        return cx == 0 ? cur : (3 * cur + row[cx - 1] + 1) >> 2;
    }
    const int cy = y >> 1;                                      // h2v2
    const u8 *near = p + (long)cy * pw;
    if (dw <= 2) return near[cx];
    int fy = (y & 1) ? cy + 1 : cy - 1;
    fy = fy < 0 ? 0 : fy > dh - 1 ? dh - 1 : fy;
    const u8 *far = p + (long)fy * pw;
    const int cur = 3 * near[cx] + far[cx];
    if (x & 1) return cx == dw - 1 ? (4 * cur + 7) >> 4 : (3 * cur + 3 * near[cx + 1] + far[cx + 1] + 7) >> 4;
    return cx == 0 ? (4 * cur + 8) >> 4 : (3 * cur + 3 * near[cx - 1] + far[cx - 1] + 8) >> 4;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// source position (x, y) in the stored W x H image of output pixel (ox, oy) under the EXIF orientation
__device__ __forceinline__ void source_xy(int orientation, int W, int H, int ox, int oy, int &x, int &y)
{
    switch (orientation) {
    case 2: x = W - 1 - ox; y = oy; break;
    case 3: x = W - 1 - ox; y = H - 1 - oy; break;
    case 4: x = ox; y = H - 1 - oy; break;
    case 5: x = oy; y = ox; break;
    case 6: x = oy; y = H - 1 - ox; break;
    case 7: x = W - 1 - oy; y = H - 1 - ox; break;
    case 8: x = W - 1 - oy; y = ox; break;
    default: x = ox; y = oy;
    }
}

// jdcolor.c: FIX(1.40200), FIX(1.77200), FIX(0.34414), FIX(0.71414); cb, cr centred on 0
__device__ __forceinline__ void store_ycc_as_bgr(u8 *px, int Y, int cb, int cr)
{
    px[0] = (u8)clamp255(Y + ((116130 * cb + 32768) >> 16));
    px[1] = (u8)clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    px[2] = (u8)clamp255(Y + ((91881 * cr + 32768) >> 16));
}

__global__ __launch_bounds__(256) void k_jpeg_colour(const u8 *__restrict__ planes, JpegColourGeom g, u8 *__restrict__ bgr, long pitch)
{
    const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y;
    if (ox >= g.OW) return;
    int x, y;
    source_xy(g.orientation, g.W, g.H, ox, oy, x, y);
    const int Y = planes[g.plane_off[0] + (long)y * g.pitch[0] + x];
    u8 *px = bgr + (long)oy * pitch + 3L * ox;
    if (g.ncomp == 3) {
        const int cb = chroma_sample(planes + g.plane_off[1], g.pitch[1], g.dw, g.dh, g.hup, g.vup, x, y) - 128;
        const int cr = chroma_sample(planes + g.plane_off[2], g.pitch[2], g.dw, g.dh, g.hup, g.vup, x, y) - 128;
        store_ycc_as_bgr(px, Y, cb, cr);
    } else {
        px[0] = px[1] = px[2] = (u8)Y;
    }
}

// the dense or the compact-form instantiation of the IDCT kernel for block size S
using IdctKernel = void (*)(const short *, const unsigned long long *, const unsigned *, const short *, const unsigned short *, JpegIdctGeom, u8 *);

template <bool SPARSE>
constexpr IdctKernel idct_kernel(int S)
{
    return S == 8 ? k_jpeg_idct<SPARSE> : S == 4 ? k_jpeg_idct4<SPARSE> : S == 2 ? k_jpeg_idct_small<2, SPARSE> : k_jpeg_idct_small<1, SPARSE>;
}

// How each component is decoded at scale 1 / denom (denom 1, 2, 4 or 8), and where its coefficients and its plane lie
struct JpegPlan {
    int sc[3];                         // block size: 8 / denom, doubled while the component is subsampled against it and it is below 8
    int bw[3], bh[3];                  // block grid (whole MCUs); 0 for a component the image does not have
    int pitch[3];                      // plane row pitch: bw * sc padded to a multiple of 4
    long coef_off[3], plane_off[3];
    long plane_bytes;
};

}  // namespace

// fn: the entry point that was called, for the error text
static int jpeg_plan(const sv_jpeg_info *info, int denom, const char *fn, JpegPlan &p)
{
    const int hmax = info->h_samp, vmax = info->v_samp, S = 8 / denom;
    const int mcu_cols = (info->width + 8 * hmax - 1) / (8 * hmax), mcu_rows = (info->height + 8 * vmax - 1) / (8 * vmax);
    long coff = 0, poff = 0;
    for (int c = 0; c < 3; c++) {
        const int h = c == 0 ? hmax : 1, v = c == 0 ? vmax : 1;
        p.sc[c] = S;                                            // jdmaster.c: decode a subsampled component larger instead of up-sampling it
        while (p.sc[c] < 8 && (hmax * S) % (h * p.sc[c] * 2) == 0 && (vmax * S) % (v * p.sc[c] * 2) == 0) p.sc[c] *= 2;
        p.bw[c] = c < info->components ? mcu_cols * h : 0;
        p.bh[c] = c < info->components ? mcu_rows * v : 0;
        p.pitch[c] = (p.bw[c] * p.sc[c] + 3) & ~3;
        p.coef_off[c] = coff; p.plane_off[c] = poff;
        coff += (long)p.bw[c] * p.bh[c] * 64;
        poff += (long)p.pitch[c] * p.bh[c] * p.sc[c];
    }
    p.plane_bytes = poff;
    if (coff != info->coef_count) return sv_fail(SV_ERR_BAD_ARG, "%s: coef_count %ld does not match the geometry (%ld)", fn, info->coef_count, coff);
    return SV_OK;
}

// bgr: ceil(out_height / denom) x ceil(out_width / denom) x 3
int svk_jpeg_reconstruct(sv_ctx *ctx, const sv_jpeg_info *info, int denom, const int16_t *coef, const uint64_t *masks, const uint32_t *offsets, const int16_t *values,
                         const uint16_t *quant, u8 *bgr, ptrdiff_t pitch, hipStream_t s, const char *fn)
{
    const int ncomp = info->components, hmax = info->h_samp, vmax = info->v_samp, S = 8 / denom;
    JpegPlan p;
    int rc = jpeg_plan(info, denom, fn, p);
    if (rc || (rc = ctx->jpeg_planes.grow(ctx, (size_t)p.plane_bytes))) return rc;   // the component planes between the IDCT and the colour kernel
    u8 *planes = ctx->jpeg_planes.as<u8>();
    for (int first = 0; first < ncomp; first++) {               // one launch per block size: luma's, then chroma's where it differs
        const int z = p.sc[first];
        if (first == 2 || (first == 1 && z == p.sc[0])) continue;
        JpegIdctGeom g = {};
        const int group = z >= 4 ? 1 : 4 / z, per_wg = z == 8 ? 32 : z == 4 ? 64 : 256;
        long items = 0;
        for (int c = 0; c < 3; c++) {
            g.bw[c] = p.bw[c]; g.bh[c] = p.sc[c] == z ? p.bh[c] : 0;
            g.ipr[c] = (p.bw[c] + group - 1) / group;
            g.pitch[c] = p.pitch[c]; g.coef_off[c] = p.coef_off[c]; g.plane_off[c] = p.plane_off[c]; g.item_start[c] = items;
            items += (long)g.ipr[c] * g.bh[c];
        }
        g.item_start[3] = items;
        const IdctKernel k = coef ? idct_kernel<false>(z) : idct_kernel<true>(z);
        hipLaunchKernelGGL(k, dim3((unsigned)((items + per_wg - 1) / per_wg)), dim3(256), 0, s, (const short *)coef, (const unsigned long long *)masks, offsets,
                           (const short *)values, quant, g, planes);
        SV_LAUNCH_CHECK("k_jpeg_idct");
    }
    JpegColourGeom cg = {};
    cg.ncomp = ncomp; cg.orientation = info->orientation;
    cg.W = (info->width + denom - 1) / denom; cg.H = (info->height + denom - 1) / denom;
    cg.OW = info->orientation >= 5 ? cg.H : cg.W; cg.OH = info->orientation >= 5 ? cg.W : cg.H;
    cg.hup = hmax * S / p.sc[1]; cg.vup = vmax * S / p.sc[1];   // full size: hmax, vmax; reduced: 2, 1 for 4:2:2 and 1, 1 otherwise
    cg.dw = S > 1 ? (info->width * p.sc[1] + hmax * 8 - 1) / (hmax * 8) : 0;    // jdsample.c: no fancy up-sampling when blocks are 1x1
    cg.dh = (info->height * p.sc[1] + vmax * 8 - 1) / (vmax * 8);
    for (int c = 0; c < 3; c++) { cg.pitch[c] = p.pitch[c]; cg.plane_off[c] = p.plane_off[c]; }
    hipLaunchKernelGGL(k_jpeg_colour, dim3((unsigned)((cg.OW + 255) / 256), (unsigned)cg.OH), dim3(256), 0, s, planes, cg, bgr, (long)pitch);
    SV_LAUNCH_CHECK("k_jpeg_colour");
    return SV_OK;
}
