// K13 -- the two full-frame passes of cv/grid_v2.py's fallback methods on MI355X.
//
//   Harris corners (detect_corners_harris, cv/grid_v2.py:272-290 = cv2.goodFeaturesToTrack(useHarrisDetector=True, blockSize 3)):
//     k_harris_response   : one 64x16 tile per workgroup.  The u8 tile with a halo of 2 is staged in LDS (BORDER_REFLECT_101 applied
//                           while loading), the Sobel derivatives Dx, Dy of the tile with a halo of 1 are computed into LDS (a
//                           derivative outside the image is the derivative AT the reflected position: the box filter reflects the
//                           covariance images, not the pixels), and every output pixel sums its nine products in double and writes
//                           the f32 response.  Each workgroup also writes the maximum of its tile.
//     k_harris_frame_max  : one workgroup per frame reduces the tile maxima (max is exact in any order).
//     k_harris_candidates : threshold at quality_level * max (double), 3x3 local-maximum test, compaction of the survivors as
//                           64-bit keys (response descending, raster index ascending) through one atomic counter per frame.
//     k_harris_select     : one workgroup per frame sorts the keys (bitonic, in place) and its first wave runs the greedy
//                           minimum-distance selection over the sorted list (64 keys per load) against the kept corners in LDS.
//   Every float operation is a separately rounded IEEE f32 operation in the order include/sudoku_vision_hip.h states
//   (the file is compiled with -ffp-contract=off; the _rn intrinsics say so at the places where it matters).
//
//   Affine warp (rotate_image, cv/grid_v2.py:371-394 = cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT)):
//     k_warp_affine       : one thread per destination pixel.  Thread 0 of a workgroup inverts the frame's forward matrix in double
//                           (cv2's sequence); coordinates in cv2's 10 + 5 bit fixed point; the bilinear sample is K2's
//                           (sv_warp_sample) inside the image and sv_remap_sample with the border constant outside.
#include "sv_device.h"
#include "sv_internal.h"

namespace {

constexpr int HT_X = 64, HT_Y = 16;               // output tile of k_harris_response
constexpr int HP_W = HT_X + 4, HP_H = HT_Y + 4;   // staged pixels
constexpr int HD_W = HT_X + 2, HD_H = HT_Y + 2;   // derivatives
constexpr int KEPT_MAX = SV_HARRIS_MAX_CORNERS;

__global__ __launch_bounds__(256) void k_harris_response(const u8 *__restrict__ img, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, float ks0, float ks1,
                                                         float k, float *__restrict__ resp, float *__restrict__ tile_max)
{
    __shared__ float px[HP_H][HP_W];
    __shared__ float dxs[HD_H][HD_W], dys[HD_H][HD_W];
    __shared__ float wmax[4];
    const int tid = threadIdx.x, frame = blockIdx.z;
    const int x0 = blockIdx.x * HT_X, y0 = blockIdx.y * HT_Y;
    const u8 *base = img + (ptrdiff_t)frame * img_stride;
    // pixels of [x0-2, x0+HT_X+2) x [y0-2, y0+HT_Y+2), reflected into the image (slots far outside it are never used)
    for (int i = tid; i < HP_H * HP_W; i += 256) {
        const int j = i / HP_W, c = i - j * HP_W;
        const int gx = x0 - 2 + c, gy = y0 - 2 + j;
        float v = 0.f;
        if (gx <= W + 1 && gy <= H + 1) v = (float)base[(ptrdiff_t)sv_reflect101(gy, H) * pitch + sv_reflect101(gx, W)];
        px[j][c] = v;
    }
    __syncthreads();
    // Dx, Dy at [x0-1, x0+HT_X+1) x [y0-1, y0+HT_Y+1); at -1 and W (H) the value at the reflected position 1 and W-2 (H-2)
    for (int i = tid; i < HD_H * HD_W; i += 256) {
        const int j = i / HD_W, c = i - j * HD_W;
        const int gx = x0 - 1 + c, gy = y0 - 1 + j;
        float dx = 0.f, dy = 0.f;
        if (gx <= W && gy <= H) {
            const int lx = sv_reflect101(gx, W) - (x0 - 2), ly = sv_reflect101(gy, H) - (y0 - 2);   // LDS position of the pixel, 1 <= l < size - 1
            // Dx: row pass p[x+1] - p[x-1] (exact), column pass ks1*S[y] + ks0*(S[y-1] + S[y+1])
            const float s0 = __fsub_rn(px[ly - 1][lx + 1], px[ly - 1][lx - 1]);
            const float s1 = __fsub_rn(px[ly][lx + 1], px[ly][lx - 1]);
            const float s2 = __fsub_rn(px[ly + 1][lx + 1], px[ly + 1][lx - 1]);
            dx = __fadd_rn(__fmul_rn(ks1, s1), __fmul_rn(ks0, __fadd_rn(s0, s2)));
            // Dy: row pass ks1*p[x] + ks0*(p[x-1] + p[x+1]), column pass S[y+1] - S[y-1]
            const float t0 = __fadd_rn(__fmul_rn(ks1, px[ly - 1][lx]), __fmul_rn(ks0, __fadd_rn(px[ly - 1][lx - 1], px[ly - 1][lx + 1])));
            const float t2 = __fadd_rn(__fmul_rn(ks1, px[ly + 1][lx]), __fmul_rn(ks0, __fadd_rn(px[ly + 1][lx - 1], px[ly + 1][lx + 1])));
            dy = __fsub_rn(t2, t0);
        }
        dxs[j][c] = dx;
        dys[j][c] = dy;
    }
    __syncthreads();
    float best = -INFINITY;
    const int tx = tid & 63;
    for (int ty = tid >> 6; ty < HT_Y; ty += 4) {
        const int gx = x0 + tx, gy = y0 + ty;
        if (gx >= W || gy >= H) continue;
        // 3x3 sums of dx*dx, dx*dy, dy*dy in double: per row left to right, then the rows top to bottom; rounded to f32 once
        double a = 0, b = 0, c = 0;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double ra = 0, rb = 0, rc = 0;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const float dx = dxs[ty + j][tx + i], dy = dys[ty + j][tx + i];
                ra = __dadd_rn(ra, (double)__fmul_rn(dx, dx));
                rb = __dadd_rn(rb, (double)__fmul_rn(dx, dy));
                rc = __dadd_rn(rc, (double)__fmul_rn(dy, dy));
            }
            a = __dadd_rn(a, ra);
            b = __dadd_rn(b, rb);
            c = __dadd_rn(c, rc);
        }
        const float fa = (float)a, fb = (float)b, fc = (float)c;
        const float tr = __fadd_rn(fa, fc);
        const float r = __fsub_rn(__fsub_rn(__fmul_rn(fa, fc), __fmul_rn(fb, fb)), __fmul_rn(__fmul_rn(k, tr), tr));
        resp[((ptrdiff_t)frame * H + gy) * W + gx] = r;
        best = fmaxf(best, r);
    }
    for (int o = 32; o > 0; o >>= 1) best = fmaxf(best, __shfl_down(best, o));
    if ((tid & 63) == 0) wmax[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) tile_max[(ptrdiff_t)frame * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}

__global__ __launch_bounds__(256) void k_harris_frame_max(const float *__restrict__ tile_max, int ntiles, float *__restrict__ frame_max, uint32_t *__restrict__ cand_count)
{
    __shared__ float wmax[4];
    const int tid = threadIdx.x, frame = blockIdx.x;
    float best = -INFINITY;
    for (int i = tid; i < ntiles; i += 256) best = fmaxf(best, tile_max[(ptrdiff_t)frame * ntiles + i]);
    for (int o = 32; o > 0; o >>= 1) best = fmaxf(best, __shfl_down(best, o));
    if ((tid & 63) == 0) wmax[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        frame_max[frame] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
        cand_count[frame] = 0;
    }
}

// A candidate's sort key: ascending key order = response descending, then raster index ascending.  Candidates are > 0, so
// their float bits order like unsigned integers.
__device__ __forceinline__ unsigned long long harris_key(float r, uint32_t index)
{
    return ((unsigned long long)(0xffffffffu - __float_as_uint(r)) << 32) | index;
}

__global__ __launch_bounds__(256) void k_harris_candidates(const float *__restrict__ resp, int H, int W, double quality, const float *__restrict__ frame_max,
                                                           uint32_t *__restrict__ cand_count, unsigned long long *__restrict__ keys, uint32_t cap, size_t key_stride)
{
    const int frame = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const float mx = frame_max[frame];
    if (!(mx > 0.f)) return;                                   // a flat frame has no corners
    if (x < 1 || y < 1 || x >= W - 1 || y >= H - 1) return;    // the outermost frame of pixels is never a corner
    const float *r = resp + (ptrdiff_t)frame * H * W;
    const float v = r[(ptrdiff_t)y * W + x];
    const double t = __dmul_rn(quality, (double)mx);
    if ((double)v < t || !(v > 0.f)) return;
    // v survives the threshold; it is a 3x3 maximum of the thresholded image iff no neighbour is larger (a neighbour below
    // the threshold counts as 0 < v)
    bool is_max = true;
#pragma unroll
    for (int j = -1; j <= 1; j++)
#pragma unroll
        for (int i = -1; i <= 1; i++) is_max = is_max && !(r[(ptrdiff_t)(y + j) * W + (x + i)] > v);
    if (!is_max) return;
    const uint32_t slot = atomicAdd(&cand_count[frame], 1u);
    if (slot < cap) keys[(size_t)frame * key_stride + slot] = harris_key(v, (uint32_t)y * (uint32_t)W + (uint32_t)x);
}

__global__ __launch_bounds__(1024) void k_harris_select(unsigned long long *__restrict__ keys, size_t key_stride, const uint32_t *__restrict__ cand_count, uint32_t cap,
                                                        int W, int max_corners, int min_dist2, float *__restrict__ corners, int *__restrict__ counts)
{
    __shared__ volatile uint32_t kept[KEPT_MAX];               // x | y << 16
    const int tid = threadIdx.x, frame = blockIdx.x;
    const uint32_t m = cand_count[frame];
    if (m > cap) {                                             // overflow: the entry reports it; no partial list
        if (tid == 0) counts[frame] = 0;
        return;
    }
    unsigned long long *kf = keys + (size_t)frame * key_stride;
    uint32_t P = 1;
    while (P < m) P <<= 1;                                     // P <= key_stride (a power of two >= cap)
    for (uint32_t i = m + tid; i < P; i += 1024) kf[i] = ~0ull;
    __syncthreads();
    for (uint32_t size = 2; size <= P; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t i = tid; i < (P >> 1); i += 1024) {
                const uint32_t lo = 2 * i - (i & (stride - 1));             // the lower index of pair i
                const uint32_t hi = lo + stride;
                const bool up = (lo & size) == 0;
                const unsigned long long a = kf[lo], b = kf[hi];
                if ((a > b) == up) { kf[lo] = b; kf[hi] = a; }
            }
            __syncthreads();
        }
    }
    if (tid >= 64) return;
    // greedy selection by the first wave: candidate after candidate, the lanes share the comparison with the kept corners
    int nkept = 0;
    for (uint32_t c0 = 0; c0 < m && nkept < max_corners; c0 += 64) {
        const uint32_t mine = c0 + tid < m ? (uint32_t)kf[c0 + tid] : 0u;     // 64 candidates per load, one per lane
        const int batch = (int)min(64u, m - c0);
        for (int j = 0; j < batch && nkept < max_corners; j++) {
            const uint32_t index = __shfl(mine, j);
            const int y = (int)(index / (uint32_t)W), x = (int)(index - (uint32_t)y * (uint32_t)W);
            bool close = false;
            if (min_dist2 > 0)
                for (int i = tid; i < nkept; i += 64) {
                    const uint32_t q = kept[i];
                    const long long dx = x - (int)(q & 0xffffu), dy = y - (int)(q >> 16);
                    close = close || dx * dx + dy * dy < (long long)min_dist2;
                }
            if (__any(close)) continue;
            if (tid == 0) {
                kept[nkept] = (uint32_t)x | ((uint32_t)y << 16);
                corners[((ptrdiff_t)frame * max_corners + nkept) * 2] = (float)x;
                corners[((ptrdiff_t)frame * max_corners + nkept) * 2 + 1] = (float)y;
            }
            nkept++;
        }
    }
    if (tid == 0) counts[frame] = nkept;
}

__global__ __launch_bounds__(256) void k_warp_affine(const u8 *__restrict__ src, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const double *__restrict__ fwd,
                                                     int dh, int dw, int border, u8 *__restrict__ dst)
{
    __shared__ double M[6];
    const int frame = blockIdx.z;
    if (threadIdx.x == 0) sv_affine_invert(fwd + (ptrdiff_t)frame * 6, M);
    __syncthreads();
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= dw || y >= dh) return;
    int X, Y, sx, sy, a, b;
    sv_affine_coord(M, x, y, X, Y);
    sv_remap_split(X, Y, sx, sy, a, b);
    const u8 *img = src + (ptrdiff_t)frame * img_stride;
    int v;
    if ((unsigned)sx < (unsigned)(W - 1) && (unsigned)sy < (unsigned)(H - 1)) {
        int out[1];
        sv_warp_sample<1>(img, H, W, pitch, sx, sy, a, b, out);
        v = out[0];
    } else {
        v = sv_remap_sample(img, H, W, pitch, sx, sy, a, b, border);
    }
    dst[((ptrdiff_t)frame * dh + y) * dw + x] = (u8)v;
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

int svk_harris_corners(sv_ctx *ctx, const u8 *gray, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int max_corners, double quality_level,
                       int min_distance, double k, int cand_capacity, float *corners, int *counts, float *response, hipStream_t s)
{
    const int tiles_x = (W + HT_X - 1) / HT_X, tiles_y = (H + HT_Y - 1) / HT_Y, ntiles = tiles_x * tiles_y;
    size_t key_stride = 1;
    while (key_stride < (size_t)cand_capacity) key_stride <<= 1;
    // scratch: response (unless the caller wants it) | tile maxima | frame maxima | candidate counts | keys
    const size_t npx = (size_t)n * H * W;
    const size_t o_tile = response ? 0 : align16(npx * sizeof(float));
    const size_t o_fmax = o_tile + align16((size_t)n * ntiles * sizeof(float));
    const size_t o_cnt = o_fmax + align16((size_t)n * sizeof(float));
    const size_t o_keys = o_cnt + align16((size_t)n * sizeof(uint32_t));
    const size_t total = o_keys + (size_t)n * key_stride * sizeof(unsigned long long);
    int rc = ctx->grid2.grow(ctx, total);
    if (rc) return rc;
    u8 *sc = ctx->grid2.as<u8>();
    float *resp = response ? response : (float *)sc;
    float *tile_max = (float *)(sc + o_tile), *frame_max = (float *)(sc + o_fmax);
    uint32_t *cand_count = (uint32_t *)(sc + o_cnt);
    unsigned long long *keys = (unsigned long long *)(sc + o_keys);

    const double scale = 1.0 / (4.0 * 3.0 * 255.0);           // Sobel normalisation of cornerHarris: 1 / (2^(ksize-1) * blockSize * 255)
    {
        sv_time_scope ts(ctx, SVK_HARRIS, s);
        hipLaunchKernelGGL(k_harris_response, dim3(tiles_x, tiles_y, n), dim3(256), 0, s, gray, H, W, pitch, img_stride, (float)scale, (float)(2.0 * scale), (float)k,
                           resp, tile_max);
        SV_LAUNCH_CHECK("k_harris_response");
        hipLaunchKernelGGL(k_harris_frame_max, dim3(n), dim3(256), 0, s, tile_max, ntiles, frame_max, cand_count);
        SV_LAUNCH_CHECK("k_harris_frame_max");
        hipLaunchKernelGGL(k_harris_candidates, dim3((W + 63) / 64, (H + 3) / 4, n), dim3(256), 0, s, resp, H, W, quality_level, frame_max, cand_count, keys,
                           (uint32_t)cand_capacity, key_stride);
        SV_LAUNCH_CHECK("k_harris_candidates");
        hipLaunchKernelGGL(k_harris_select, dim3(n), dim3(1024), 0, s, keys, key_stride, cand_count, (uint32_t)cand_capacity, W, max_corners,
                           min_distance > 0 ? min_distance * min_distance : 0, corners, counts);
        SV_LAUNCH_CHECK("k_harris_select");
    }
    // the candidate counts decide the status: a frame with more candidates than the capacity fails the call
    std::vector<uint32_t> host_count(n);
    SV_HIP(hipMemcpyAsync(host_count.data(), cand_count, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s));
    SV_HIP(hipStreamSynchronize(s));
    for (int f = 0; f < n; f++)
        if (host_count[f] > (uint32_t)cand_capacity)
            return sv_fail(SV_ERR_BUFFER, "sv_harris_corners_u8: frame %d has %u corner candidates, capacity %d", f, host_count[f], cand_capacity);
    return SV_OK;
}

int svk_warp_affine(sv_ctx *ctx, const u8 *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const double *fwd, int dh, int dw, int border, u8 *dst,
                    hipStream_t s)
{
    sv_time_scope ts(ctx, SVK_WARP_AFFINE, s);
    hipLaunchKernelGGL(k_warp_affine, dim3((dw + 63) / 64, (dh + 3) / 4, n), dim3(256), 0, s, src, H, W, pitch, img_stride, fwd, dh, dw, border, dst);
    SV_LAUNCH_CHECK("k_warp_affine");
    return SV_OK;
}
