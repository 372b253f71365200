// Device-side building blocks shared by the K1/K2 kernels and the K3 fc heads.  Integer stages are exact by
// construction; float/double stages use the _rn intrinsics so that no multiply-add is ever fused
// (the arithmetic being matched rounds after every operation).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

typedef uint8_t u8;

// cv2.cvtColor(BGR2GRAY), 15-bit coefficients (cv/preprocess.py:19, cv/extract.py:49).
__device__ __forceinline__ int sv_gray_px(int b, int g, int r)
{
    return (b * 3735 + g * 19235 + r * 9798 + 16384) >> 15;
}

__device__ __forceinline__ int sv_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The normalise glue between an 8-bit cell and the CNN input: x = ((255 - cell)/255 - 0.5)/0.5, one rounding per operation
// (pipeline/run.py:129-135, pipeline/run_v2.py:161-163)
__device__ __forceinline__ float sv_glue_norm(u8 c)
{
    const float t = __fdiv_rn((float)(255 - (int)c), 255.0f);
    return __fdiv_rn(__fsub_rn(t, 0.5f), 0.5f);
}

// cv2 BORDER_REFLECT_101
__device__ __forceinline__ int sv_reflect101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

// cv2's saturate_cast<int>(double): round half to even, saturating
__device__ __forceinline__ int sv_sat_int(double v) { return __double2int_rn(fmax(-2147483648.0, fmin(2147483647.0, v))); }

// The tail of every cv2 remap: coordinates (X, Y) with INTER_BITS = 5 fractional bits -> source cell (sx, sy), saturated to
// int16 as cv2 stores it, and the 1/32 fractions (a, b).
__device__ __forceinline__ void sv_remap_split(int X, int Y, int &sx, int &sy, int &a, int &b)
{
    sx = sv_clamp(X >> 5, -32768, 32767);
    sy = sv_clamp(Y >> 5, -32768, 32767);
    a = X & 31;
    b = Y & 31;
}

// Width of the column blocks cv2.warpPerspective evaluates its fp64 coordinates in.
__host__ __device__ __forceinline__ int sv_warp_block_w(int dw, int dh)
{
    int bh0 = 16 < dh ? 16 : dh;
    int bw0 = 1024 / bh0 < dw ? 1024 / bh0 : dw;
    return bw0;
}

// cv2.warpPerspective evaluates the homography at the origin (x0, dy) of each 64-column block of a destination row in double and
// steps from there: these three values depend on the block and the row only.
__device__ __forceinline__ void sv_warp_block_origin(const double *M, int x0, int dy, double &X0, double &Y0, double &W0)
{
    const double fx0 = (double)x0, fy = (double)dy;
    X0 = __dadd_rn(__dadd_rn(__dmul_rn(M[0], fx0), __dmul_rn(M[1], fy)), M[2]);
    Y0 = __dadd_rn(__dadd_rn(__dmul_rn(M[3], fx0), __dmul_rn(M[4], fy)), M[5]);
    W0 = __dadd_rn(__dadd_rn(__dmul_rn(M[6], fx0), __dmul_rn(M[7], fy)), M[8]);
}

// Destination pixel x1 columns right of a block origin -> source cell (sx,sy) and 1/32 fractions (a,b), cv/grid.py:131.
__device__ __forceinline__ void sv_warp_coord_from(const double *M, double X0, double Y0, double W0, int x1, int &sx, int &sy, int &a, int &b)
{
    const double fx1 = (double)x1;
    double Wv = __dadd_rn(W0, __dmul_rn(M[6], fx1));
    Wv = Wv != 0.0 ? __ddiv_rn(32.0, Wv) : 0.0;
    double fX = __dmul_rn(__dadd_rn(X0, __dmul_rn(M[0], fx1)), Wv);
    double fY = __dmul_rn(__dadd_rn(Y0, __dmul_rn(M[3], fx1)), Wv);
    fX = fmax(-2147483648.0, fmin(2147483647.0, fX));
    fY = fmax(-2147483648.0, fmin(2147483647.0, fY));
    sv_remap_split(__double2int_rn(fX), __double2int_rn(fY), sx, sy, a, b);
}

// Destination pixel (dx,dy) -> source cell (sx,sy) and 1/32 fractions (a,b)
__device__ __forceinline__ void sv_warp_coord(const double *M, int dx, int dy, int bw, int &sx, int &sy, int &a, int &b)
{
    const int x0 = (dx / bw) * bw;
    double X0, Y0, W0;
    sv_warp_block_origin(M, x0, dy, X0, Y0, W0);
    sv_warp_coord_from(M, X0, Y0, W0, dx - x0, sx, sy, a, b);
}

__device__ __forceinline__ int sv_tap(const u8 *img, int H, int W, ptrdiff_t pitch, int C, int x, int y, int c)
{
    if ((unsigned)x >= (unsigned)W || (unsigned)y >= (unsigned)H) return 0;
    return img[(ptrdiff_t)y * pitch + (ptrdiff_t)x * C + c];
}

// One bilinear sample at source cell (sx,sy) with fractions (a,b)/32: 15-bit weights (they sum to 32768), constant-0 border.
template <int C>
__device__ __forceinline__ void sv_warp_sample(const u8 *img, int H, int W, ptrdiff_t pitch, int sx, int sy, int a, int b, int (&out)[C]);

template <int C>
__device__ __forceinline__ void sv_warp_px(const u8 *img, int H, int W, ptrdiff_t pitch, const double *M, int dx, int dy,
                                           int bw, int (&out)[C])
{
    int sx, sy, a, b;
    sv_warp_coord(M, dx, dy, bw, sx, sy, a, b);
    sv_warp_sample<C>(img, H, W, pitch, sx, sy, a, b, out);
}

template <int C>
__device__ __forceinline__ void sv_warp_sample(const u8 *img, int H, int W, ptrdiff_t pitch, int sx, int sy, int a, int b, int (&out)[C])
{
    const int w00 = (32 - a) * (32 - b) * 32, w01 = a * (32 - b) * 32, w10 = (32 - a) * b * 32, w11 = a * b * 32;
    const bool inside = (unsigned)sx < (unsigned)(W - 1) && (unsigned)sy < (unsigned)(H - 1);
    if (inside) {
        const u8 *p0 = img + (ptrdiff_t)sy * pitch + (ptrdiff_t)sx * C;
        const u8 *p1 = p0 + pitch;
#pragma unroll
        for (int c = 0; c < C; c++)
            out[c] = (p0[c] * w00 + p0[C + c] * w01 + p1[c] * w10 + p1[C + c] * w11 + 16384) >> 15;
    } else {
#pragma unroll
        for (int c = 0; c < C; c++)
            out[c] = (sv_tap(img, H, W, pitch, C, sx, sy, c) * w00 + sv_tap(img, H, W, pitch, C, sx + 1, sy, c) * w01 +
                      sv_tap(img, H, W, pitch, C, sx, sy + 1, c) * w10 + sv_tap(img, H, W, pitch, C, sx + 1, sy + 1, c) * w11 +
                      16384) >> 15;
    }
}

// One single-channel bilinear sample of cv2.remap at source cell (sx, sy), fractions (a, b) / 32, wherever the cell lies.  border < 0
// is BORDER_REPLICATE: each tap's coordinates clamped; border >= 0 is BORDER_CONSTANT: a tap outside the image reads `border`.
// Every load is at a clamped position, so none leaves the image.  Pitch is int for a dense plane in LDS, ptrdiff_t for a
// pitched global image.
// cv2's weight table is (32-a)(32-b)*32, a(32-b)*32, (32-a)b*32, ab*32 but for a = b = 0, where 32768 saturates to 32767 and the
// table's correction puts the missing 1 on the last tap: (32767 p00 + p11 + 16384) >> 15 = p00 for 8-bit values, the same as
// these weights give.
template <class Pitch>
__device__ __forceinline__ int sv_remap_sample(const u8 *img, int H, int W, Pitch pitch, int sx, int sy, int a, int b, int border)
{
    const int w00 = (32 - a) * (32 - b) * 32, w01 = a * (32 - b) * 32, w10 = (32 - a) * b * 32, w11 = a * b * 32;
    const int x0 = sv_clamp(sx, 0, W - 1), x1 = sv_clamp(sx + 1, 0, W - 1), y0 = sv_clamp(sy, 0, H - 1), y1 = sv_clamp(sy + 1, 0, H - 1);
    int t00 = img[(Pitch)y0 * pitch + x0], t01 = img[(Pitch)y0 * pitch + x1], t10 = img[(Pitch)y1 * pitch + x0], t11 = img[(Pitch)y1 * pitch + x1];
    if (border >= 0) {
        const bool xi0 = x0 == sx, xi1 = x1 == sx + 1, yi0 = y0 == sy, yi1 = y1 == sy + 1;       // the tap lies inside iff its clamp moved nothing
        if (!(xi0 && yi0)) t00 = border;
        if (!(xi1 && yi0)) t01 = border;
        if (!(xi0 && yi1)) t10 = border;
        if (!(xi1 && yi1)) t11 = border;
    }
    return (t00 * w00 + t01 * w01 + t10 * w10 + t11 * w11 + 16384) >> 15;
}

// cv2.warpAffine without WARP_INVERSE_MAP inverts the forward 2x3 matrix m by this sequence of double operations (a singular
// matrix gives zeros) -> M[0..5]
__device__ __forceinline__ void sv_affine_invert(const double *m, double *M)
{
    double D = __dsub_rn(__dmul_rn(m[0], m[4]), __dmul_rn(m[1], m[3]));
    D = D != 0.0 ? __ddiv_rn(1.0, D) : 0.0;
    const double A11 = __dmul_rn(m[4], D), A22 = __dmul_rn(m[0], D);
    const double m1 = __dmul_rn(m[1], -D), m3 = __dmul_rn(m[3], -D);
    M[0] = A11; M[1] = m1; M[3] = m3; M[4] = A22;
    M[2] = __dsub_rn(__dmul_rn(-A11, m[2]), __dmul_rn(m1, m[5]));
    M[5] = __dsub_rn(__dmul_rn(-m3, m[2]), __dmul_rn(A22, m[5]));
}

// Destination pixel (x, y) of cv2.warpAffine under the inverse matrix M -> source coordinates (X, Y) with 5 fractional bits, for
// sv_remap_split.  AB_BITS = 10: 1/1024 px coordinates, + 16 rounds the >> 5 that leaves 5 fractional bits; the sums wrap as cv2's do.
__device__ __forceinline__ void sv_affine_coord(const double *M, int x, int y, int &X, int &Y)
{
    const double fx = (double)x, fy = (double)y;
    const int adelta = sv_sat_int(__dmul_rn(__dmul_rn(M[0], fx), 1024.0)), bdelta = sv_sat_int(__dmul_rn(__dmul_rn(M[3], fx), 1024.0));
    const int X0 = (int)((unsigned)sv_sat_int(__dmul_rn(__dadd_rn(__dmul_rn(M[1], fy), M[2]), 1024.0)) + 16u);
    const int Y0 = (int)((unsigned)sv_sat_int(__dmul_rn(__dadd_rn(__dmul_rn(M[4], fy), M[5]), 1024.0)) + 16u);
    X = (int)((unsigned)X0 + (unsigned)adelta) >> 5;
    Y = (int)((unsigned)Y0 + (unsigned)bdelta) >> 5;
}

// cv2.resize INTER_LINEAR 8-bit axis table entry (cv/extract.py:52): source offset + two 11-bit weights.
// scale = 1 / (d_len / s_len), two double divisions (sv_resize_axis below, or the same two on the host: IEEE either way).
__device__ __forceinline__ void sv_resize_axis_scaled(double scale, int d, int &ofs, int &w0, int &w1)
{
    float f = (float)__dadd_rn(__dmul_rn(__dadd_rn((double)d, 0.5), scale), -0.5);
    const int s = (int)floorf(f);
    f = __fsub_rn(f, (float)s);
    ofs = s;
    w0 = __float2int_rn(__fmul_rn(__fsub_rn(1.f, f), 2048.f));
    w1 = __float2int_rn(__fmul_rn(f, 2048.f));
}

__device__ __forceinline__ void sv_resize_axis(int s_len, int d_len, int d, int &ofs, int &w0, int &w1)
{
    sv_resize_axis_scaled(__ddiv_rn(1.0, __ddiv_rn((double)d_len, (double)s_len)), d, ofs, w0, w1);
}

// One pixel of 8-bit cv2.resize(INTER_LINEAR) from its axis entries (xo, a0, a1), (yo, b0, b1) over an sh x sw source whose
// pixel (x, y) is tap(x, y): a column left of the image or on its last column takes weights (2048, 0), the rows are clamped, and
// the blend has cv2's two stages.  Every tap lies inside the source.
template <class Tap>
__device__ __forceinline__ int sv_resize_px(int xo, int a0, int a1, int yo, int b0, int b1, int sh, int sw, Tap tap)
{
    if (xo < 0) { xo = 0; a0 = 2048; a1 = 0; }
    if (xo >= sw - 1) { xo = sw - 1; a0 = 2048; a1 = 0; }
    const int x1 = xo + 1 < sw ? xo + 1 : xo;
    const int y0 = sv_clamp(yo, 0, sh - 1), y1 = sv_clamp(yo + 1, 0, sh - 1);
    const int t0 = tap(xo, y0) * a0 + tap(x1, y0) * a1;
    const int t1 = tap(xo, y1) * a0 + tap(x1, y1) * a1;
    return (((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2;
}

// ---- the fc2 -> argmax -> softmax[argmax] epilogue of every fc head (pipeline/run.py:139-143), in f32 on the VALU ----
// fc2.weight [10][128] -> w2s (LDS), by the NTHREADS threads of the workgroup
template <int NTHREADS>
__device__ __forceinline__ void sv_fc2_stage(float (*w2s)[128], const float *w2, int tid)
{
    for (int i = tid; i < 1280; i += NTHREADS) w2s[i >> 7][i & 127] = w2[i];
}

// logit j of a cell from its 128 hidden activations h: b2[j] + h . w2s[j], one fmaf per term in order n = 0..127
__device__ __forceinline__ float sv_fc2_logit(const float *h, const float (*w2s)[128], const float *b2, int j)
{
    float s = b2[j];
    for (int n = 0; n < 128; n++) s = __builtin_fmaf(h[n], w2s[j][n], s);
    return s;
}

// index of the first maximum of the 10 logits lg; best = that maximum
__device__ __forceinline__ int sv_argmax10(const float *lg, float &best)
{
    best = lg[0];
    int arg = 0;
    for (int j = 1; j < 10; j++)
        if (lg[j] > best) { best = lg[j]; arg = j; }
    return arg;
}

// digit (first maximum of the 10 logits lg) and confidence (its softmax probability, 1 / sum exp(lg - best)) of cell `cell`
__device__ __forceinline__ void sv_digit_conf(const float *lg, long cell, u8 *digits, float *conf)
{
    if (!digits && !conf) return;
    float best;
    const int arg = sv_argmax10(lg, best);
    if (digits) digits[cell] = (u8)arg;
    if (conf) {
        float den = 0.f;
        for (int j = 0; j < 10; j++) den += expf(lg[j] - best);
        conf[cell] = 1.0f / den;
    }
}

// the same with a temperature (ml/model_v3.py:216-225): the digit is the argmax of lg, the confidence softmax(lg / temperature) at it,
// every logit divided before the subtraction
__device__ __forceinline__ void sv_digit_conf_t(const float *lg, float temperature, long cell, u8 *digits, float *conf)
{
    if (!digits && !conf) return;
    float best;
    const int arg = sv_argmax10(lg, best);
    if (digits) digits[cell] = (u8)arg;
    if (conf) {
        best = best / temperature;
        float den = 0.f;
        for (int j = 0; j < 10; j++) den += expf(lg[j] / temperature - best);
        conf[cell] = 1.0f / den;
    }
}
