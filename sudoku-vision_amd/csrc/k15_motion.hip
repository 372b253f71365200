// K15 -- cv/stabilizer.py:264-291 (MotionDetector.update) for n consecutive frames of one feed on MI355X.
//
//   small[i]  = cv2.resize(gray(frames[i]), (dw, dh)): only the taps the resize reads are converted to gray (cvtColor is pointwise, so
//               this is the same byte as resizing the whole gray image); no full-size intermediate exists.
//   counts[i] = pixels with |small[i] - small[i-1]| > threshold, small[-1] = prev_small (none: counts[0] = 0).
//
// One thread per pixel of a small image, a workgroup inside one frame (blockIdx.y).  The resize has three forms, chosen per launch:
// the 11-bit table (any size, up- or downscaling; the axis entries are recomputed per thread from the two scales the host divides
// once), the copy (source already dh x dw) and cv2's 2x2 area mean (source exactly 2 dh x 2 dw: resize.cpp turns INTER_LINEAR into
// INTER_AREA there).  The count is a wave ballot + popcount, summed over the workgroup's four waves in LDS, one integer atomic per
// workgroup: the order cannot matter.
//
// Frame i's difference needs frame i-1's small image.  Two launch shapes compute it (DESIGN section 20 has the measurement):
//   k_motion<C, true>                     one launch: the thread computes its pixel of frame i-1 again from that frame's taps (for
//                                         i = 0 it reads prev_small).  A single frame never recomputes anything.
//   k_motion<C, false> + k_motion_count   two launches: every small image is written first, the second pass reads them back.
#include "sv_device.h"
#include "sv_internal.h"

namespace {

constexpr int MT = 256;                       // threads per workgroup
enum { RESIZE_TABLE = 0, RESIZE_COPY = 1, RESIZE_AREA2 = 2 };

struct motion_geom {
    int H, W, dh, dw, form;
    double scale_x, scale_y;                  // 1 / (dw / W), 1 / (dh / H)
    ptrdiff_t pitch, frame_stride;
};

template <int C>
__device__ __forceinline__ int gray_tap(const u8 *img, ptrdiff_t pitch, int x, int y)
{
    const u8 *p = img + (ptrdiff_t)y * pitch + (ptrdiff_t)x * C;
    return C == 3 ? sv_gray_px(p[0], p[1], p[2]) : p[0];
}

// pixel (x, y) of cv2.resize(gray(img), (dw, dh)); every tap lies inside the H x W image
template <int C>
__device__ __forceinline__ int small_px(const u8 *img, const motion_geom &g, int x, int y)
{
    if (g.form == RESIZE_COPY) return gray_tap<C>(img, g.pitch, x, y);
    if (g.form == RESIZE_AREA2)
        return (gray_tap<C>(img, g.pitch, 2 * x, 2 * y) + gray_tap<C>(img, g.pitch, 2 * x + 1, 2 * y) +
                gray_tap<C>(img, g.pitch, 2 * x, 2 * y + 1) + gray_tap<C>(img, g.pitch, 2 * x + 1, 2 * y + 1) + 2) >> 2;
    int xo, a0, a1, yo, b0, b1;
    sv_resize_axis_scaled(g.scale_x, x, xo, a0, a1);
    sv_resize_axis_scaled(g.scale_y, y, yo, b0, b1);
    return sv_resize_px(xo, a0, a1, yo, b0, b1, g.H, g.W, [&](int tx, int ty) { return gray_tap<C>(img, g.pitch, tx, ty); });
}

// counts[frame] += the workgroup's threads with `moved` set.  Every thread of the workgroup calls it.
__device__ __forceinline__ void count_moved(bool moved, int32_t *counts, int frame)
{
    __shared__ int part[MT / 64];
    const int c = __popcll(__ballot(moved));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < MT / 64; w++) s += part[w];
        if (s) atomicAdd(&counts[frame], s);
    }
}

// thr: a difference d counts iff d > thr (integer; the host turns the float threshold into it)
template <int C, bool COUNT>
__global__ __launch_bounds__(MT) void k_motion(const u8 *__restrict__ frames, motion_geom g, const u8 *__restrict__ prev_small, int thr,
                                               u8 *__restrict__ small, int32_t *__restrict__ counts)
{
    const int npx = g.dh * g.dw, p = blockIdx.x * MT + threadIdx.x, frame = blockIdx.y;
    const bool active = p < npx;
    bool moved = false;
    if (active) {
        const int y = p / g.dw, x = p - y * g.dw;
        const u8 *img = frames + (ptrdiff_t)frame * g.frame_stride;
        const int cur = small_px<C>(img, g, x, y);
        small[(ptrdiff_t)frame * npx + p] = (u8)cur;
        if (COUNT && (frame > 0 || prev_small)) {
            const int prev = frame > 0 ? small_px<C>(img - g.frame_stride, g, x, y) : prev_small[p];
            moved = abs(cur - prev) > thr;
        }
    }
    if (COUNT) count_moved(moved, counts, frame);
}

__global__ __launch_bounds__(MT) void k_motion_count(const u8 *__restrict__ small, const u8 *__restrict__ prev_small, int npx, int thr,
                                                     int32_t *__restrict__ counts)
{
    const int p = blockIdx.x * MT + threadIdx.x, frame = blockIdx.y;
    bool moved = false;
    if (p < npx && (frame > 0 || prev_small)) {
        const u8 *cur = small + (ptrdiff_t)frame * npx;
        const int prev = frame > 0 ? cur[p - (ptrdiff_t)npx] : prev_small[p];
        moved = abs((int)cur[p] - prev) > thr;
    }
    count_moved(moved, counts, frame);
}

// Zeroes the counts the workgroups add into.  A kernel and not hipMemsetAsync: captured into a graph, a memset of 16 bytes or more
// was carried out on the first replay only, and these 4n bytes reach that at four frames.
__global__ __launch_bounds__(MT) void k_motion_clear(int32_t *__restrict__ counts, int n)
{
    const int i = blockIdx.x * MT + threadIdx.x;
    if (i < n) counts[i] = 0;
}

}  // namespace

// A u8 difference d against a float threshold t: d > t  <=>  d > floor(t) for finite t; NaN and t >= 255 count nothing, t < 0 everything.
static int integer_threshold(float t)
{
    if (!(t < 255.f)) return 255;
    if (t < 0.f) return -1;
    return (int)t;
}

int svk_motion_update(sv_ctx *ctx, const u8 *frames, int n, int H, int W, int C, ptrdiff_t pitch, ptrdiff_t frame_stride, const u8 *prev_small,
                      float threshold, u8 *small, int32_t *counts, int dh, int dw, hipStream_t s)
{
    motion_geom g;
    g.H = H; g.W = W; g.dh = dh; g.dw = dw;
    g.form = H == dh && W == dw ? RESIZE_COPY : (H == 2 * (long)dh && W == 2 * (long)dw ? RESIZE_AREA2 : RESIZE_TABLE);
    g.scale_x = 1.0 / ((double)dw / (double)W);
    g.scale_y = 1.0 / ((double)dh / (double)H);
    g.pitch = pitch; g.frame_stride = frame_stride;
    const int npx = dh * dw, thr = integer_threshold(threshold);
    const dim3 grid((unsigned)((npx + MT - 1) / MT), (unsigned)n);
    // one launch unless the cross-check library asks for the other shape (svx_ctx_set_motion_shape); a single frame has nothing to recompute
    const bool two_pass = n > 1 && ctx->x_motion_shape == 1;
    hipLaunchKernelGGL(k_motion_clear, dim3((unsigned)((n + MT - 1) / MT)), dim3(MT), 0, s, counts, n);
    SV_LAUNCH_CHECK("k_motion_clear");
    if (two_pass) {
        if (C == 3) hipLaunchKernelGGL((k_motion<3, false>), grid, dim3(MT), 0, s, frames, g, prev_small, thr, small, counts);
        else        hipLaunchKernelGGL((k_motion<1, false>), grid, dim3(MT), 0, s, frames, g, prev_small, thr, small, counts);
        SV_LAUNCH_CHECK("k_motion");
        hipLaunchKernelGGL(k_motion_count, grid, dim3(MT), 0, s, small, prev_small, npx, thr, counts);
        SV_LAUNCH_CHECK("k_motion_count");
    } else {
        if (C == 3) hipLaunchKernelGGL((k_motion<3, true>), grid, dim3(MT), 0, s, frames, g, prev_small, thr, small, counts);
        else        hipLaunchKernelGGL((k_motion<1, true>), grid, dim3(MT), 0, s, frames, g, prev_small, thr, small, counts);
        SV_LAUNCH_CHECK("k_motion");
    }
    return SV_OK;
}
