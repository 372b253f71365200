// K7 -- the whole-frame pixel work of cv/preprocess_v2.py (pipeline/run_v2.py:278-280) on MI355X.  Every stage is integer, or
// float32 with one rounding per operation (the _rn intrinsics: nothing is ever fused), so each has exactly one right answer.
//
//   k_morph_element       rows of a RECT / ELLIPSE structuring element (cv2.getStructuringElement) as column spans
//   k_morph_planes<MAX>   horizontal doubling planes P_l(x,y) = max|min src(x .. x+2^l-1, y), l = 1..L, one row segment per
//                         workgroup, built level by level through the LDS
//   k_morph_gather<MAX>   dilate / erode: an element row is one span, a span maximum is the max of two overlapping power-of-two
//                         windows, so a pixel costs 2 reads per element row: O(k), not O(k^2); scratch is L = floor(log2 k) planes
//   k_box<MODE>           k x k window sums (BORDER_REFLECT_101) by sliding column sums marching down a strip and a workgroup
//                         prefix scan across them; MODE = the rounded mean (cv2.blur) or the Sauvola decision
//   k_gauss21             cv2.GaussianBlur(21,21,0) on u8: 8-bit fixed-point taps, exact horizontal pass into LDS, vertical pass
//   k_clahe_hist/_lut/_apply   cv2.createCLAHE(clip, (tx,ty)).apply for any size: tile histograms (LDS, merged by integer
//                         atomics), clip + redistribute + CDF by one workgroup per tile, bilinear LUT blend in float32
//   k_pointwise<MODE>     the per-pixel tails: division by the background, fixed thresholds, the shadow mask, and per-frame
//                         counts of the pixels set (integer atomics)
//
// Sources may have any pitch / frame stride / alignment (byte loads only); every output is dense [n][H][W].
#include <algorithm>

#include "sv_device.h"
#include "sv_internal.h"

namespace {

// cv2 borderInterpolate(BORDER_REFLECT_101) for any distance from the image (windows larger than the image)
__device__ __forceinline__ int reflect101(int p, int len)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    const int period = 2 * len - 2;
    int m = p % period;
    if (m < 0) m += period;
    return m < len ? m : period - m;
}

// ---- morphology ---------------------------------------------------------------------------------------------------------
constexpr int MORPH_MAX_K = 4095;
constexpr int MT = 1024;          // pixels of a row per k_morph_planes workgroup

// element row i -> the columns it covers relative to the pixel, [x, y] inclusive (anchor (k/2, k/2) subtracted)
__global__ void k_morph_element(int shape, int k, short2 *rows)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= k) return;
    const int anchor = k / 2;
    int j0 = 0, j1 = k;
    if (shape == SV_SHAPE_ELLIPSE) {
        const int r = k / 2, c = k / 2, dy = i - r;
        const double inv_r2 = r ? __ddiv_rn(1.0, (double)(r * r)) : 0.0;
        const int dx = __double2int_rn(__dmul_rn((double)c, __dsqrt_rn(__dmul_rn((double)(r * r - dy * dy), inv_r2))));
        j0 = max(c - dx, 0);
        j1 = min(c + dx + 1, k);
    }
    rows[i] = make_short2((short)(j0 - anchor), (short)(j1 - 1 - anchor));
}

template <bool MAX>
__device__ __forceinline__ int mm(int a, int b) { return MAX ? max(a, b) : min(a, b); }

// planes + (l-1) * plane_bytes = P_l, dense [n][H][W]; pixels right of the image do not take part (identity)
template <bool MAX>
__global__ __launch_bounds__(256) void k_morph_planes(const u8 *__restrict__ src, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int nlev,
                                                      u8 *__restrict__ planes, size_t plane_bytes)
{
    extern __shared__ u8 sm[];
    const int span = MT + (1 << nlev), tid = threadIdx.x;
    u8 *a = sm, *b = sm + span;
    const int x0 = blockIdx.x * MT, y = blockIdx.y, f = blockIdx.z;
    const u8 *row = src + (ptrdiff_t)f * img_stride + (ptrdiff_t)y * pitch;
    for (int i = tid; i < span; i += 256) a[i] = x0 + i < W ? row[x0 + i] : (u8)(MAX ? 0 : 255);
    __syncthreads();
    for (int l = 0; l < nlev; l++) {
        const int step = 1 << l;
        for (int i = tid; i + step < span; i += 256) b[i] = (u8)mm<MAX>(a[i], a[i + step]);
        __syncthreads();
        u8 *out = planes + (size_t)l * plane_bytes + ((size_t)f * H + y) * W + x0;
        for (int i = tid; i < MT && x0 + i < W; i += 256) out[i] = b[i];
        u8 *t = a; a = b; b = t;
    }
}

template <bool MAX>
__global__ __launch_bounds__(256) void k_morph_gather(const u8 *__restrict__ src, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride,
                                                      const u8 *__restrict__ planes, size_t plane_bytes, const short2 *__restrict__ rows, int k,
                                                      u8 *__restrict__ dst)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, f = blockIdx.z;
    if (x >= W || y >= H) return;
    const int ay = k / 2;
    const u8 *img = src + (ptrdiff_t)f * img_stride;
    const int i0 = max(0, ay - y), i1 = min(k, H + ay - y);        // element rows that land inside the image
    int v = MAX ? 0 : 255;
    for (int i = i0; i < i1; i++) {
        const short2 r = rows[i];
        const int a = max(x + r.x, 0), b = min(x + r.y, W - 1);
        if (a > b) continue;
        const int l = 31 - __clz(b - a + 1), yy = y + i - ay;
        int p, q;
        if (l == 0) {
            p = q = img[(ptrdiff_t)yy * pitch + a];
        } else {
            const u8 *pr = planes + (size_t)(l - 1) * plane_bytes + ((size_t)f * H + yy) * W;
            p = pr[a];
            q = pr[b - (1 << l) + 1];
        }
        v = mm<MAX>(v, mm<MAX>(p, q));
    }
    dst[((size_t)f * H + y) * W + x] = (u8)v;
}

// ---- k x k window sums --------------------------------------------------------------------------------------------------
constexpr int BT = 512;                 // output columns per workgroup
constexpr int BR = 64;                  // rows per workgroup (the first row costs k rows of reads, each later one 2)
constexpr int BOX_MAX_K = 1023;
constexpr int BNC = BT + BOX_MAX_K - 1; // columns incl. halo
enum { BOX_MEAN = 0, BOX_SAUVOLA = 1 };

template <int MODE>
__global__ __launch_bounds__(256) void k_box(const u8 *__restrict__ src, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int w, double inv_area,
                                             float kf, u8 *__restrict__ dst)
{
    constexpr bool SQ = MODE == BOX_SAUVOLA;
    __shared__ uint32_t cs1[BNC], cs2[SQ ? BNC : 1];                 // column sums of g and g^2 over the window's rows
    __shared__ uint32_t p1[BNC + 1];                                 // exclusive prefix sums across the columns
    __shared__ unsigned long long p2[SQ ? BNC + 1 : 1];
    __shared__ uint32_t wt1[4];
    __shared__ unsigned long long wt2[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = w / 2, x0 = blockIdx.x * BT, y0 = blockIdx.y * BR, f = blockIdx.z;
    const int nout = min(BT, W - x0), ncols = nout + 2 * r, y1 = min(H, y0 + BR);
    const u8 *img = src + (ptrdiff_t)f * img_stride;
    for (int j = tid; j < ncols; j += 256) {
        const int xs = reflect101(x0 - r + j, W);
        uint32_t s1 = 0, s2 = 0;
        for (int dy = -r; dy <= r; dy++) {
            const uint32_t g = img[(ptrdiff_t)reflect101(y0 + dy, H) * pitch + xs];
            s1 += g;
            s2 += g * g;
        }
        cs1[j] = s1;
        if (SQ) cs2[j] = s2;
    }
    const int chunk = (ncols + 255) / 256, cb = min(tid * chunk, ncols), ce = min(cb + chunk, ncols);
    for (int y = y0; y < y1; y++) {
        __syncthreads();
        uint32_t t1 = 0;
        unsigned long long t2 = 0;
        for (int j = cb; j < ce; j++) {
            t1 += cs1[j];
            if (SQ) t2 += cs2[j];
        }
        uint32_t i1 = t1;
        unsigned long long i2 = t2;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u1 = __shfl_up(i1, o);
            const unsigned long long u2 = SQ ? __shfl_up(i2, o) : 0;
            if (lane >= o) { i1 += u1; i2 += u2; }
        }
        if (lane == 63) { wt1[wave] = i1; wt2[wave] = i2; }
        __syncthreads();
        uint32_t e1 = i1 - t1;
        unsigned long long e2 = i2 - t2;
        for (int k = 0; k < wave; k++) { e1 += wt1[k]; e2 += wt2[k]; }
        for (int j = cb; j < ce; j++) {
            p1[j] = e1;
            e1 += cs1[j];
            if (SQ) { p2[j] = e2; e2 += cs2[j]; }
        }
        if (ce == ncols && cb < ce) {
            p1[ncols] = e1;
            if (SQ) p2[ncols] = e2;
        }
        __syncthreads();
        for (int xo = tid; xo < nout; xo += 256) {
            const uint32_t S1 = p1[xo + w] - p1[xo];
            u8 out;
            if (MODE == BOX_MEAN) {
                const uint32_t area = (uint32_t)(w * w);
                out = (u8)((2 * S1 + area) / (2 * area));
            } else {
                const unsigned long long S2 = p2[xo + w] - p2[xo];
                const float mean = __double2float_rn(__dmul_rn((double)S1, inv_area));
                const float sq = __double2float_rn(__dmul_rn((double)S2, inv_area));
                const float var = fmaxf(__fsub_rn(sq, __fmul_rn(mean, mean)), 0.f);
                const float sd = __fsqrt_rn(var);
                const float t = __fmul_rn(mean, __fadd_rn(1.f, __fmul_rn(kf, __fsub_rn(__fdiv_rn(sd, 128.f), 1.f))));
                out = (float)img[(ptrdiff_t)y * pitch + x0 + xo] < t ? 255 : 0;
            }
            dst[((size_t)f * H + y) * W + x0 + xo] = out;
        }
        __syncthreads();
        if (y + 1 < y1) {                                        // slide the column sums one row down
            const ptrdiff_t add = (ptrdiff_t)reflect101(y + 1 + r, H) * pitch, sub = (ptrdiff_t)reflect101(y - r, H) * pitch;
            for (int j = tid; j < ncols; j += 256) {
                const int xs = reflect101(x0 - r + j, W);
                const uint32_t ga = img[add + xs], gs = img[sub + xs];
                cs1[j] += ga - gs;
                if (SQ) cs2[j] += ga * ga - gs * gs;
            }
        }
    }
}

// ---- GaussianBlur(21, 21, 0) on u8 --------------------------------------------------------------------------------------
// sigma 3.5, taps x 256 by error diffusion from the ends inward, centre = 256 - the rest (tests/test_preprocess_v2_ref.py pins them)
__device__ constexpr int G21[21] = {0, 2, 2, 4, 6, 11, 15, 20, 25, 28, 30, 28, 25, 20, 15, 11, 6, 4, 2, 2, 0};
constexpr int GW = 64, GH = 32;

__global__ __launch_bounds__(256) void k_gauss21(const u8 *__restrict__ src, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, u8 *__restrict__ dst)
{
    __shared__ unsigned short hs[GH + 20][GW];
    const int tid = threadIdx.x, x0 = blockIdx.x * GW, y0 = blockIdx.y * GH, f = blockIdx.z;
    const u8 *img = src + (ptrdiff_t)f * img_stride;
    for (int idx = tid; idx < (GH + 20) * GW; idx += 256) {
        const int ry = idx / GW, rx = idx % GW, x = x0 + rx;
        int s = 0;
        if (x < W) {
            const u8 *row = img + (ptrdiff_t)reflect101(y0 - 10 + ry, H) * pitch;
            if (x >= 10 && x + 10 < W) {
#pragma unroll
                for (int t = 0; t < 21; t++) s += G21[t] * row[x - 10 + t];
            } else {
#pragma unroll
                for (int t = 0; t < 21; t++) s += G21[t] * row[reflect101(x - 10 + t, W)];
            }
        }
        hs[ry][rx] = (unsigned short)s;                          // <= 255 * 256
    }
    __syncthreads();
    for (int idx = tid; idx < GH * GW; idx += 256) {
        const int ry = idx / GW, rx = idx % GW, x = x0 + rx, y = y0 + ry;
        if (x >= W || y >= H) continue;
        int s = 0;
#pragma unroll
        for (int t = 0; t < 21; t++) s += G21[t] * hs[ry + t][rx];
        dst[((size_t)f * H + y) * W + x] = (u8)((s + 32768) >> 16);
    }
}

// ---- CLAHE --------------------------------------------------------------------------------------------------------------
constexpr int CLAHE_ROWS = 32;      // tile rows per k_clahe_hist workgroup

// Zeroes the tile histograms, one per workgroup.  A kernel and not hipMemsetAsync: captured into a graph, that memset zeroed the
// histograms on the first replay only (tests/test_gpu_stream_order.py), and a launch replays like every other launch of the entry.
__global__ __launch_bounds__(256) void k_clahe_clear(uint32_t *__restrict__ hist)
{
    hist[(size_t)blockIdx.x * 256 + threadIdx.x] = 0;
}

// The image is extended to a multiple of the tile grid at the bottom and the right with BORDER_REFLECT_101 (never written out).
__global__ __launch_bounds__(256) void k_clahe_hist(const u8 *__restrict__ src, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int tiles_x, int tw,
                                                    int th, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t h[256];
    const int tid = threadIdx.x, tile = blockIdx.x, f = blockIdx.z;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int r0 = blockIdx.y * CLAHE_ROWS, r1 = min(th, r0 + CLAHE_ROWS);
    h[tid] = 0;
    __syncthreads();
    const u8 *img = src + (ptrdiff_t)f * img_stride;
    for (int r = r0; r < r1; r++) {
        const u8 *row = img + (ptrdiff_t)reflect101(ty * th + r, H) * pitch;
        for (int c = tid; c < tw; c += 256) atomicAdd(&h[row[reflect101(tx * tw + c, W)]], 1u);
    }
    __syncthreads();
    if (h[tid]) atomicAdd(&hist[((size_t)f * gridDim.x + tile) * 256 + tid], h[tid]);
}

__global__ __launch_bounds__(256) void k_clahe_lut(const uint32_t *__restrict__ hist, int clip_limit, float lut_scale, u8 *__restrict__ lut)
{
    __shared__ int s[256];
    const int i = threadIdx.x;
    int h = (int)hist[(size_t)blockIdx.x * 256 + i];
    if (clip_limit > 0) {
        s[i] = h > clip_limit ? h - clip_limit : 0;
        h = min(h, clip_limit);
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (i < o) s[i] += s[i + o];
            __syncthreads();
        }
        const int clipped = s[0], batch = clipped / 256, residual = clipped - batch * 256;
        __syncthreads();
        h += batch;
        if (residual != 0) {
            const int step = max(256 / residual, 1);
            if (i % step == 0 && i / step < residual) h++;
        }
    }
    s[i] = h;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                           // inclusive scan
        const int v = i >= o ? s[i - o] : 0;
        __syncthreads();
        s[i] += v;
        __syncthreads();
    }
    const int v = __float2int_rn(__fmul_rn((float)s[i], lut_scale));
    lut[(size_t)blockIdx.x * 256 + i] = (u8)sv_clamp(v, 0, 255);
}

__global__ __launch_bounds__(256) void k_clahe_apply(const u8 *__restrict__ src, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int tiles_x, int tiles_y,
                                                     float inv_tw, float inv_th, const u8 *__restrict__ luts, u8 *__restrict__ dst)
{
    const int x = blockIdx.x * 64 + threadIdx.x, f = blockIdx.z;
    if (x >= W) return;
    const float txf = __fsub_rn(__fmul_rn((float)x, inv_tw), 0.5f);
    int tx1 = (int)floorf(txf);
    const float xa = __fsub_rn(txf, (float)tx1), xa1 = __fsub_rn(1.f, xa);
    const int tx2 = min(tx1 + 1, tiles_x - 1);
    tx1 = max(tx1, 0);
    const u8 *lut = luts + (size_t)f * tiles_x * tiles_y * 256;
    const u8 *img = src + (ptrdiff_t)f * img_stride;
    for (int k = 0; k < 8; k++) {
        const int y = (blockIdx.y * 4 + threadIdx.y) * 8 + k;
        if (y >= H) return;
        const float tyf = __fsub_rn(__fmul_rn((float)y, inv_th), 0.5f);
        int ty1 = (int)floorf(tyf);
        const float ya = __fsub_rn(tyf, (float)ty1), ya1 = __fsub_rn(1.f, ya);
        const int ty2 = min(ty1 + 1, tiles_y - 1);
        ty1 = max(ty1, 0);
        const int v = img[(ptrdiff_t)y * pitch + x];
        const float l11 = lut[(ty1 * tiles_x + tx1) * 256 + v], l12 = lut[(ty1 * tiles_x + tx2) * 256 + v];
        const float l21 = lut[(ty2 * tiles_x + tx1) * 256 + v], l22 = lut[(ty2 * tiles_x + tx2) * 256 + v];
        const float top = __fadd_rn(__fmul_rn(l11, xa1), __fmul_rn(l12, xa)), bot = __fadd_rn(__fmul_rn(l21, xa1), __fmul_rn(l22, xa));
        const float res = __fadd_rn(__fmul_rn(top, ya1), __fmul_rn(bot, ya));
        dst[((size_t)f * H + y) * W + x] = (u8)sv_clamp(__float2int_rn(res), 0, 255);
    }
}

// ---- per-pixel tails ----------------------------------------------------------------------------------------------------
enum { PW_DIVIDE = 0, PW_BINARY = 1, PW_BINARY_INV = 2, PW_SHADOW = 3, PW_COUNT = 4 };

// Zeroes the per-frame counts k_pointwise adds into: a kernel for the reason k_clahe_clear is one (4n bytes reach 16 at four frames).
__global__ __launch_bounds__(256) void k_counts_clear(uint32_t *__restrict__ counts, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) counts[i] = 0;
}

// a workgroup covers 64 x 32 pixels; `other` (dense) is the background (PW_DIVIDE) or the local mean (PW_SHADOW); counts[f] += pixels set
template <int MODE>
__global__ __launch_bounds__(256) void k_pointwise(const u8 *__restrict__ src, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride,
                                                   const u8 *__restrict__ other, int param, u8 *__restrict__ dst, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t part[4];
    const int x = blockIdx.x * 64 + threadIdx.x, f = blockIdx.z;
    const u8 *img = src + (ptrdiff_t)f * img_stride;
    uint32_t cnt = 0;
    if (x < W) {
        for (int k = 0; k < 8; k++) {
            const int y = (blockIdx.y * 4 + threadIdx.y) * 8 + k;
            if (y >= H) break;
            const size_t o = ((size_t)f * H + y) * W + x;
            const int g = img[(ptrdiff_t)y * pitch + x];
            int out;
            if (MODE == PW_DIVIDE) {
                const float q = __fmul_rn(__fdiv_rn((float)g, (float)max((int)other[o], 1)), 255.f);
                out = (int)fminf(fmaxf(q, 0.f), 255.f);
            } else if (MODE == PW_BINARY) {
                out = g > param ? 255 : 0;
            } else if (MODE == PW_BINARY_INV) {
                out = g > param ? 0 : 255;
            } else if (MODE == PW_SHADOW) {
                out = g - (int)other[o] < param ? 255 : 0;
            } else {
                out = g;
            }
            if (MODE != PW_COUNT) dst[o] = (u8)out;
            cnt += out != 0;
        }
    }
    if (MODE == PW_DIVIDE) return;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
    if (threadIdx.x == 0) part[threadIdx.y] = cnt;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        const uint32_t t = part[0] + part[1] + part[2] + part[3];
        if (t) atomicAdd(&counts[f], t);
    }
}

template <bool MAX>
int morph_once(const u8 *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int nlev, u8 *planes, const short2 *rows, int k, u8 *dst,
               hipStream_t s)
{
    const size_t plane_bytes = (size_t)n * H * W;
    if (nlev > 0) {
        hipLaunchKernelGGL(k_morph_planes<MAX>, dim3((W + MT - 1) / MT, H, n), dim3(256), 2 * (size_t)(MT + (1 << nlev)), s, src, H, W, pitch, img_stride, nlev,
                           planes, plane_bytes);
        SV_LAUNCH_CHECK("k_morph_planes");
    }
    hipLaunchKernelGGL(k_morph_gather<MAX>, dim3((W + 63) / 64, (H + 3) / 4, n), dim3(64, 4), 0, s, src, H, W, pitch, img_stride, planes, plane_bytes, rows, k, dst);
    SV_LAUNCH_CHECK("k_morph_gather");
    return SV_OK;
}

template <int MODE>
int pointwise(const u8 *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const u8 *other, int param, u8 *dst, uint32_t *counts, hipStream_t s)
{
    if (counts) {
        hipLaunchKernelGGL(k_counts_clear, dim3((n + 255) / 256), dim3(256), 0, s, counts, n);
        SV_LAUNCH_CHECK("k_counts_clear");
    }
    hipLaunchKernelGGL(k_pointwise<MODE>, dim3((W + 63) / 64, (H + 31) / 32, n), dim3(64, 4), 0, s, src, H, W, pitch, img_stride, other, param, dst, counts);
    SV_LAUNCH_CHECK("k_pointwise");
    return SV_OK;
}

}  // namespace

int svk_morphology(sv_ctx *ctx, const u8 *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int op, int shape, int k, u8 *dst, hipStream_t s)
{
    if (k > MORPH_MAX_K) return sv_fail(SV_ERR_UNSUPPORTED, "sv_morphology_u8: ksize %d > %d", k, MORPH_MAX_K);
    // the longest span that can lie inside the image decides how many doubling planes are needed
    int nlev = 0;
    while ((2 << nlev) <= std::min(k, W)) nlev++;
    const size_t plane_bytes = (size_t)n * H * W, rows_bytes = ((size_t)k * sizeof(short2) + 255) / 256 * 256;
    const bool two = op == SV_MORPH_CLOSE || op == SV_MORPH_OPEN;
    int rc = ctx->pp2.grow(ctx, rows_bytes + plane_bytes * (nlev + (two ? 1 : 0)));
    if (rc) return rc;
    u8 *base = ctx->pp2.as<u8>();
    short2 *rows = (short2 *)base;
    u8 *planes = base + rows_bytes, *mid = planes + plane_bytes * nlev;
    hipLaunchKernelGGL(k_morph_element, dim3((k + 255) / 256), dim3(256), 0, s, shape, k, rows);
    SV_LAUNCH_CHECK("k_morph_element");
    const ptrdiff_t dp = W, ds = (ptrdiff_t)H * W;
    switch (op) {
    case SV_MORPH_DILATE: return morph_once<true>(src, n, H, W, pitch, img_stride, nlev, planes, rows, k, dst, s);
    case SV_MORPH_ERODE:  return morph_once<false>(src, n, H, W, pitch, img_stride, nlev, planes, rows, k, dst, s);
    case SV_MORPH_CLOSE:
        if ((rc = morph_once<true>(src, n, H, W, pitch, img_stride, nlev, planes, rows, k, mid, s))) return rc;
        return morph_once<false>(mid, n, H, W, dp, ds, nlev, planes, rows, k, dst, s);
    default:
        if ((rc = morph_once<false>(src, n, H, W, pitch, img_stride, nlev, planes, rows, k, mid, s))) return rc;
        return morph_once<true>(mid, n, H, W, dp, ds, nlev, planes, rows, k, dst, s);
    }
}

int svk_box_mean(const u8 *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int k, u8 *dst, hipStream_t s)
{
    if (k > BOX_MAX_K) return sv_fail(SV_ERR_UNSUPPORTED, "sv_box_mean_u8: ksize %d > %d", k, BOX_MAX_K);
    hipLaunchKernelGGL(k_box<BOX_MEAN>, dim3((W + BT - 1) / BT, (H + BR - 1) / BR, n), dim3(256), 0, s, src, H, W, pitch, img_stride, k, 0.0, 0.f, dst);
    SV_LAUNCH_CHECK("k_box");
    return SV_OK;
}

int svk_threshold_sauvola(const u8 *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int window, double k, u8 *dst, hipStream_t s)
{
    if (window > BOX_MAX_K) return sv_fail(SV_ERR_UNSUPPORTED, "sv_threshold_sauvola_u8: window %d > %d", window, BOX_MAX_K);
    const double inv_area = 1.0 / (double)(window * window);
    hipLaunchKernelGGL(k_box<BOX_SAUVOLA>, dim3((W + BT - 1) / BT, (H + BR - 1) / BR, n), dim3(256), 0, s, src, H, W, pitch, img_stride, window, inv_area,
                       (float)k, dst);
    SV_LAUNCH_CHECK("k_box");
    return SV_OK;
}

int svk_gaussian_blur21(const u8 *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, u8 *dst, hipStream_t s)
{
    hipLaunchKernelGGL(k_gauss21, dim3((W + GW - 1) / GW, (H + GH - 1) / GH, n), dim3(256), 0, s, src, H, W, pitch, img_stride, dst);
    SV_LAUNCH_CHECK("k_gauss21");
    return SV_OK;
}

int svk_clahe(sv_ctx *ctx, const u8 *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, double clip, int tiles_x, int tiles_y, u8 *dst, hipStream_t s)
{
    const int We = W % tiles_x ? W + tiles_x - W % tiles_x : W, He = H % tiles_y ? H + tiles_y - H % tiles_y : H;
    const int tw = We / tiles_x, th = He / tiles_y, area = tw * th, ntiles = tiles_x * tiles_y;
    int clip_limit = 0;
    if (clip > 0.0) clip_limit = std::max((int)(clip * area / 256), 1);
    const float lut_scale = 255.0f / (float)area, inv_tw = 1.0f / (float)tw, inv_th = 1.0f / (float)th;
    const size_t hist_bytes = (size_t)n * ntiles * 256 * sizeof(uint32_t);
    const int rc = ctx->pp2.grow(ctx, hist_bytes + (size_t)n * ntiles * 256);
    if (rc) return rc;
    u8 *base = ctx->pp2.as<u8>();
    uint32_t *hist = (uint32_t *)base;
    u8 *luts = base + hist_bytes;
    hipLaunchKernelGGL(k_clahe_clear, dim3(n * ntiles), dim3(256), 0, s, hist);
    SV_LAUNCH_CHECK("k_clahe_clear");
    hipLaunchKernelGGL(k_clahe_hist, dim3(ntiles, (th + CLAHE_ROWS - 1) / CLAHE_ROWS, n), dim3(256), 0, s, src, H, W, pitch, img_stride, tiles_x, tw, th, hist);
    SV_LAUNCH_CHECK("k_clahe_hist");
    hipLaunchKernelGGL(k_clahe_lut, dim3(n * ntiles), dim3(256), 0, s, hist, clip_limit, lut_scale, luts);
    SV_LAUNCH_CHECK("k_clahe_lut");
    hipLaunchKernelGGL(k_clahe_apply, dim3((W + 63) / 64, (H + 31) / 32, n), dim3(64, 4), 0, s, src, H, W, pitch, img_stride, tiles_x, tiles_y, inv_tw, inv_th,
                       luts, dst);
    SV_LAUNCH_CHECK("k_clahe_apply");
    return SV_OK;
}

int svk_divide_normalize(const u8 *gray, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const u8 *background, u8 *dst, hipStream_t s)
{
    return pointwise<PW_DIVIDE>(gray, n, H, W, pitch, img_stride, background, 0, dst, nullptr, s);
}

int svk_threshold_count(const u8 *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int thresh, int type_inv, u8 *dst, uint32_t *counts, hipStream_t s)
{
    return type_inv ? pointwise<PW_BINARY_INV>(src, n, H, W, pitch, img_stride, nullptr, thresh, dst, counts, s)
                    : pointwise<PW_BINARY>(src, n, H, W, pitch, img_stride, nullptr, thresh, dst, counts, s);
}

int svk_shadow_mask(const u8 *gray, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const u8 *local_mean, int delta, u8 *mask, uint32_t *counts, hipStream_t s)
{
    return pointwise<PW_SHADOW>(gray, n, H, W, pitch, img_stride, local_mean, delta, mask, counts, s);
}

int svk_count_nonzero(const u8 *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, uint32_t *counts, hipStream_t s)
{
    return pointwise<PW_COUNT>(src, n, H, W, pitch, img_stride, nullptr, 0, nullptr, counts, s);
}
