// The inverse DCTs of the JPEG decoders, shared by the colour path (k5_jpeg.hip) and the luma-only path (k20_jpeg_gray.hip): dequantisation
// of dense or compact-form blocks and libjpeg's 8x8 (jidctint.c), 4x4, 2x2 and 1x1 (jidctred.c) transforms up to the range-limited samples.
// One arithmetic, pinned bit-exact against libjpeg-turbo by the tests of both paths; what differs between the kernels is where a block comes
// from (their front) and where its samples go (their back).
#pragma once
#include "sv_internal.h"

namespace {

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

// The block bodies.  blk (dense) or mask + vals (SPARSE) name one block, q its component's 64 quantiser steps; they are read only where `live`.

// S = 8.  Eight threads per block, 32 blocks per workgroup of 256: the caller is thread r of block slot b.  Coefficients come in as one 16-byte
// load per thread (a block row), are dequantised into LDS, transformed in place column-wise then row-wise (LDS rows padded to 9 words: both
// passes conflict-free).  Returns the eight samples of block row r, four to a word.  Two barriers: every thread of the workgroup calls it.
template <bool SPARSE>
__device__ __forceinline__ void jpeg_idct8_row(int (&ws)[32][8][9], int b, int r, bool live, const short *__restrict__ blk, unsigned long long mask,
                                               const short *__restrict__ vals, const unsigned short *__restrict__ q, unsigned &lo, unsigned &hi)
{
    if (live) {
        int d[8];
        deq_row<SPARSE, 0xFFu>(blk, mask, vals, q, r, d);
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
    lo = hi = 0;
    if (live) {                                                 // pass 2: row r
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = ws[b][r][i];
        idct8(v, o);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            lo |= range_limit(descale(o[i], 18)) << (8 * i);
            hi |= range_limit(descale(o[4 + i], 18)) << (8 * i);
        }
    }
}

// S = 4.  Four threads per block, 64 blocks per workgroup of 256: the caller is thread t of block slot b.  It dequantises block rows t and t + 4
// into LDS, transforms columns t and t + 4, then row t; row and column 4 are never touched.  Returns the four samples of block row t.  Two
// barriers: every thread of the workgroup calls it.  ws: [block][row * 9 + column]; 73: neighbouring blocks start 9 banks apart.
template <bool SPARSE>
__device__ __forceinline__ unsigned jpeg_idct4_row(int (&ws)[64][73], int b, int t, bool live, const short *__restrict__ blk, unsigned long long mask,
                                                   const short *__restrict__ vals, const unsigned short *__restrict__ q)
{
    if (live) {
#pragma unroll
        for (int h = 0; h < 2; h++) {                           // rows t and t + 4, never row 4
            const int row = t + 4 * h;
            if (row == 4) continue;
            int d[8];
            deq_row<SPARSE, 0xEFu>(blk, mask, vals, q, row, d);
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
    unsigned w = 0;
    if (live) {                                                 // pass 2: row t
#pragma unroll
        for (int i = 0; i < 8; i++) if (i != 4) v[i] = ws[b][t * 9 + i];
        idct4(v, o);
#pragma unroll
        for (int i = 0; i < 4; i++) w |= range_limit(descale(o[i], 19)) << (8 * i);
    }
    return w;
}

// S = 2: a whole block in one thread's registers; rows and columns 0, 1, 3, 5, 7 are read.  The two samples of each row, low byte first, are
// OR-ed into top and bottom `shift` bits up.
template <bool SPARSE>
__device__ __forceinline__ void jpeg_idct2_block(const short *__restrict__ blk, unsigned long long mask, const short *__restrict__ vals,
                                                 const unsigned short *__restrict__ q, int shift, unsigned &top, unsigned &bottom)
{
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
    top |= (range_limit(descale(o0, 20)) | range_limit(descale(o1, 20)) << 8) << shift;
    idct2(w1[0], w1[1], w1[3], w1[5], w1[7], o0, o1);
    bottom |= (range_limit(descale(o0, 20)) | range_limit(descale(o1, 20)) << 8) << shift;
}

// S = 1: the DC term alone.  Zigzag position 0 is the DC term: the block's first value when present.
template <bool SPARSE>
__device__ __forceinline__ unsigned jpeg_idct1_block(const short *__restrict__ blk, unsigned long long mask, const short *__restrict__ vals,
                                                     const unsigned short *__restrict__ q)
{
    const int dc = SPARSE ? ((mask & 1) ? (int)vals[0] : 0) : (int)blk[0];
    return range_limit(descale(dc * (int)q[0], 3));
}

}  // namespace
