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
#include "sv_jpeg_idct.h"               // the transforms themselves, shared with the luma-only decoder (k20_jpeg_gray.hip)

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
    const long gb = g.coef_off[c] / 64 + lb;                    // block index over all components
    unsigned lo, hi;
    jpeg_idct8_row<SPARSE>(ws, b, r, live, SPARSE ? nullptr : coef + gb * 64, SPARSE && live ? masks[gb] : 0, SPARSE && live ? values + offsets[gb] : nullptr,
                           quant + c * 64, lo, hi);
    if (live) {
        const int bx = (int)(lb % g.bw[c]), by = (int)(lb / g.bw[c]);
        *(uint2 *)(planes + g.plane_off[c] + ((long)by * 8 + r) * g.pitch[c] + bx * 8) = make_uint2(lo, hi);
    }
}

template <bool SPARSE>
__global__ __launch_bounds__(256) void k_jpeg_idct4(const short *__restrict__ coef, const unsigned long long *__restrict__ masks,
                                                     const unsigned *__restrict__ offsets, const short *__restrict__ values,
                                                     const unsigned short *__restrict__ quant, JpegIdctGeom g, u8 *__restrict__ planes)
{
    __shared__ int ws[64][73];
    const int tid = threadIdx.x, b = tid >> 2, t = tid & 3;
    const long item = (long)blockIdx.x * 64 + b;
    const bool live = item < g.item_start[3];
    const int c = live ? component_of(g, item) : 0;
    const long lb = item - g.item_start[c];                     // block index within the component
    const long gb = g.coef_off[c] / 64 + lb;                    // block index over all components
    const unsigned w = jpeg_idct4_row<SPARSE>(ws, b, t, live, SPARSE ? nullptr : coef + gb * 64, SPARSE && live ? masks[gb] : 0,
                                              SPARSE && live ? values + offsets[gb] : nullptr, quant + c * 64);
    if (live) {
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
        if (S == 1) word[0] |= jpeg_idct1_block<SPARSE>(blk, mask, vals, q) << (8 * j);
        else jpeg_idct2_block<SPARSE>(blk, mask, vals, q, 16 * j, word[0], word[S - 1]);
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
