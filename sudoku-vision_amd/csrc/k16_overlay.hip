// K16 -- the solved digits drawn into the camera frame on MI355X: the "AR overlay" of the reference's roadmap
// (ios/.../SolutionOverlayView.swift places the digits with an identity transform; pipeline/overlay.py:63-71 has the colours).
//
// The picture is defined in include/sudoku_vision_hip.h (sv_render_overlay_u8): two 450 x 450 coverage layers that are never
// materialised -- A, the glyph of every drawn cell, and B, A moved 2 texels right and down and halved (the drop shadow) -- are
// warped into the W x H frame with cv2.warpPerspective's fixed-point arithmetic (sv_device.h: sv_warp_block_origin,
// sv_warp_coord_from; here the frame is the destination and M, frame -> grid, is the matrix the coordinates are computed with),
// and blended over the frame in integers.
//
// One workgroup of 256 threads per block of bh = min(16,H) rows by bw = min(1024/bh, W) columns of the frame, counted from the
// frame's origin: cv2's own block, so the block origin's X0, Y0, W0 depend on the row only (a wave of the 64 x 16 block walks one
// row at a time, lane = column).  The launch draws in place; sv_render_overlay_u8 copies the frames first when dst != frames.
//
// Work region.  A pixel needs arithmetic only if one of its taps can be non-zero.  Glyphs are zero in rows and columns 0..2 and
// 47..49, so A is non-zero only at layer coordinates 3..446 and B only at 5..448.
//   * per block (block_reaches_grid): M is evaluated at the block's four corner pixels.  Where W has one sign there, it has it in
//     the whole block (W is affine), the block maps onto the convex hull of the four images, and if the hull's bounding box misses
//     [-1, 450]^2 no pixel of the block can have a tap in 2..449: the fixed-point coordinate is within 1/64 texel plus float64
//     rounding of the exact one, and the guards on |W| keep that rounding below 1e-6 texel (DESIGN.md has the argument).  Such a
//     block ends without touching memory.  A block where W changes sign, is tiny against its terms or is not finite is processed.
//   * per pixel: the source cell (sx, sy) itself decides, exactly: the taps are at sx, sx+1 and sy, sy+1, and for the shadow two
//     texels up and left of them, so outside 2 <= sx, sy <= 448 every tap is zero.
//   * a pixel whose a and s both come out 0 is not loaded or stored: (f*255 + 127)/255 = f.
// Every non-zero tap of a pixel, shadow taps included, lies >= 3 texels inside the cell that holds the top-left tap (a tap in a
// neighbouring cell is in that cell's zero margin), so one digit, one class and one glyph serve the pixel; glyph coordinates
// outside [0,50) read 0, which is what the neighbour's margin holds.
#include "sv_device.h"
#include "sv_internal.h"

namespace {

constexpr int OT = 256;                                         // threads per workgroup
constexpr int GRID = SV_OVERLAY_GRID, CELL = SV_OVERLAY_CELL;
constexpr int ATLAS_BYTES = 9 * CELL * CELL;
constexpr u8 DEFAULT_PALETTE[9] = {255, 100, 0, 0, 0, 0, 0, 0, 255};   // BGR: solved, original, low confidence (pipeline/overlay.py:63-71)

struct overlay_geom {
    int H, W, bh, bw, k;
    ptrdiff_t pitch, img_stride;
    bool shadow;
};

// Can a pixel of the block [x0,x1] x [y0,y1] (inclusive pixel coordinates) have a non-zero tap?  false only when provably not.
__device__ __forceinline__ bool block_reaches_grid(const double *M, int x0, int y0, int x1, int y1)
{
    double umin = 0, umax = 0, vmin = 0, vmax = 0, wmin = 0, smax = 0, sw = 0;
    bool neg = false;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const double x = (double)((c & 1) ? x1 : x0), y = (double)((c & 2) ? y1 : y0);
        const double X = M[0] * x + M[1] * y + M[2], Y = M[3] * x + M[4] * y + M[5], Wv = M[6] * x + M[7] * y + M[8];
        const double sxy = fabs(M[0] * x) + fabs(M[1] * y) + fabs(M[2]) + fabs(M[3] * x) + fabs(M[4] * y) + fabs(M[5]);
        const double swv = fabs(M[6] * x) + fabs(M[7] * y) + fabs(M[8]);
        if (!(fabs(Wv) <= 1.7e308) || !(sxy <= 1.7e308)) return true;   // NaN or infinite
        const double u = X / Wv, v = Y / Wv;
        if (c == 0) {
            neg = Wv < 0;
            umin = umax = u; vmin = vmax = v; wmin = fabs(Wv); smax = sxy; sw = swv;
        } else {
            if ((Wv < 0) != neg) return true;
            umin = fmin(umin, u); umax = fmax(umax, u); vmin = fmin(vmin, v); vmax = fmax(vmax, v);
            wmin = fmin(wmin, fabs(Wv)); smax = fmax(smax, sxy); sw = fmax(sw, swv);
        }
    }
    // |W| against the terms it is summed from (its relative rounding error stays below 1e-9) and against those of X and Y (their
    // absolute rounding error, divided by W, stays below 1e-6 texel); !(>) so that a zero W is processed
    if (!(wmin > 1e-6 * sw) || !(wmin > 1e-9 * smax)) return true;
    return !(umax < -1.0 || umin > (double)GRID || vmax < -1.0 || vmin > (double)GRID);
}

// coverage texel (gy, gx) of a glyph; outside the glyph 0 (there the layer holds a neighbour's zero margin, or nothing)
__device__ __forceinline__ int glyph_tap(const u8 *glyph, int gy, int gx)
{
    return ((unsigned)gy < (unsigned)CELL && (unsigned)gx < (unsigned)CELL) ? glyph[gy * CELL + gx] : 0;
}

__global__ __launch_bounds__(OT) void k_overlay(u8 *__restrict__ img, overlay_geom g, const double *__restrict__ m, const u8 *__restrict__ digits,
                                                const u8 *__restrict__ classes, const u8 *__restrict__ atlas, const u8 *__restrict__ palette,
                                                const u8 *__restrict__ active)
{
    const int frame = blockIdx.z;
    if (active && !active[frame]) return;
    double M[9];
#pragma unroll
    for (int i = 0; i < 9; i++) M[i] = m[(size_t)frame * 9 + i];
    const int x0 = blockIdx.x * g.bw, y0 = blockIdx.y * g.bh;
    const int bw = min(g.bw, g.W - x0), bh = min(g.bh, g.H - y0);
    if (!block_reaches_grid(M, x0, y0, x0 + bw - 1, y0 + bh - 1)) return;
    u8 *base = img + (ptrdiff_t)frame * g.img_stride;
    const u8 *dig = digits + (size_t)frame * 81, *cls = classes ? classes + (size_t)frame * 81 : nullptr;
    // g.bw is 64 for every frame of 16 rows or more: p / g.bw is then the row, the same for a whole wave
    for (int p = threadIdx.x; p < g.bw * bh; p += OT) {
        const int ry = p / g.bw, x1 = p - ry * g.bw;
        if (x1 >= bw) continue;
        const int y = y0 + ry;
        double X0, Y0, W0;
        sv_warp_block_origin(M, x0, y, X0, Y0, W0);
        int sx, sy, a, b;
        sv_warp_coord_from(M, X0, Y0, W0, x1, sx, sy, a, b);
        if (sx < 2 || sx > GRID - 2 || sy < 2 || sy > GRID - 2) continue;
        const int cy = sy / CELL, cx = sx / CELL, cell = cy * 9 + cx;
        const int d = dig[cell], c = cls ? cls[cell] : 0;
        if (d < 1 || d > 9 || c >= g.k) continue;
        const u8 *glyph = atlas + (d - 1) * (CELL * CELL);
        const int gy = sy - cy * CELL, gx = sx - cx * CELL;
        const int w00 = (32 - a) * (32 - b) * 32, w01 = a * (32 - b) * 32, w10 = (32 - a) * b * 32, w11 = a * b * 32;
        const int av = (glyph_tap(glyph, gy, gx) * w00 + glyph_tap(glyph, gy, gx + 1) * w01 + glyph_tap(glyph, gy + 1, gx) * w10 +
                        glyph_tap(glyph, gy + 1, gx + 1) * w11 + 16384) >> 15;
        int sv = 0;
        if (g.shadow)
            sv = ((glyph_tap(glyph, gy - 2, gx - 2) >> 1) * w00 + (glyph_tap(glyph, gy - 2, gx - 1) >> 1) * w01 +
                  (glyph_tap(glyph, gy - 1, gx - 2) >> 1) * w10 + (glyph_tap(glyph, gy - 1, gx - 1) >> 1) * w11 + 16384) >> 15;
        if ((av | sv) == 0) continue;
        u8 *px = base + (ptrdiff_t)y * g.pitch + (ptrdiff_t)(x0 + x1) * 3;
        const u8 *col = palette + c * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const int t = (px[ch] * (255 - sv) + 127) / 255;
            px[ch] = (u8)((t * (255 - av) + col[ch] * av + 127) / 255);
        }
    }
}

}  // namespace

int svk_set_overlay_glyphs(sv_ctx *ctx, const u8 *atlas)
{
    const int rc = ctx->overlay.grow(ctx, ATLAS_BYTES + sizeof DEFAULT_PALETTE);
    if (rc) return rc;
    ctx->overlay_set = false;
    SV_HIP(hipSetDevice(ctx->device));
    // synchronous copies: a launch that still reads the old atlas finishes first
    SV_HIP(hipDeviceSynchronize());
    SV_HIP(hipMemcpy(ctx->overlay.p, atlas, ATLAS_BYTES, hipMemcpyHostToDevice));
    SV_HIP(hipMemcpy(ctx->overlay.as<u8>() + ATLAS_BYTES, DEFAULT_PALETTE, sizeof DEFAULT_PALETTE, hipMemcpyHostToDevice));
    ctx->overlay_set = true;
    return SV_OK;
}

int svk_render_overlay(sv_ctx *ctx, u8 *img, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const double *m, const u8 *digits, const u8 *classes,
                       const u8 *palette, int k, const u8 *active, bool shadow, hipStream_t s)
{
    overlay_geom g;
    g.H = H; g.W = W; g.k = k; g.shadow = shadow;
    g.bh = H < 16 ? H : 16;
    g.bw = sv_warp_block_w(W, H);
    g.pitch = pitch; g.img_stride = img_stride;
    const u8 *atlas = ctx->overlay.as<u8>();
    const dim3 grid((unsigned)((W + g.bw - 1) / g.bw), (unsigned)((H + g.bh - 1) / g.bh), (unsigned)n);
    hipLaunchKernelGGL(k_overlay, grid, dim3(OT), 0, s, img, g, m, digits, classes, atlas, palette ? palette : atlas + ATLAS_BYTES, active);
    SV_LAUNCH_CHECK("k_overlay");
    return SV_OK;
}
