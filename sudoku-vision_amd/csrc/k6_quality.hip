// K6 -- the integer statistics behind cv/grid_quality.py:48-149 (assess_grid_quality's per-pixel metrics) on MI355X.
//
//   k_frame_quality_stats<C,VEC> : per frame, over gray = BGR2GRAY(frame) (or the frame itself, C = 1):
//                                  lap_sum = sum(L), lap_sqsum = sum(L^2) of the 3x3 Laplacian [0 1 0; 1 -4 1; 0 1 0] with
//                                  BORDER_REFLECT_101 (cv2.Laplacian, ksize 1), and the 256-bin gray histogram.  Integer
//                                  only, so the atomics that merge partial sums cannot change a bit.
//   k_grid_line_coverage<BITS>   : per (frame, band), how many of the band's warped pixels are > 0 -- compute_completeness's
//                                  20 bands of the 450x450 warp, warped pixel by pixel with sv_warp_px's arithmetic and never
//                                  materialised.  BITS: the source is a bit image (sv_preprocess_bits_u8's layout).
//
// Stats layout: one wave per item = (frame, 1024-px column tile, QROWS-row segment).  A lane owns 16 adjacent pixels of every
// row of its segment and marches down it holding the gray values of rows y-1, y, y+1 in registers; the horizontal neighbours
// of its first and last pixel come from the adjacent lanes (shuffles), or from memory at tile and frame edges.  Histogram:
// QCOPIES sub-histograms per wave in LDS (copy = lane % QCOPIES, bins interleaved) so that a paper frame's few hot bins do
// not serialise one wave's ds_add; each wave merges its own non-zero bins into the frame's global histogram once.
#include "sv_device.h"
#include "sv_internal.h"

namespace {

constexpr int QP = 16;            // pixels per lane
constexpr int QTILE = 64 * QP;    // pixels per wave row
constexpr int QROWS = 32;         // rows per wave item
constexpr int QCOPIES = 4;        // LDS sub-histograms per wave

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int C>
__device__ __forceinline__ int gray_at(const u8 *row, int x)
{
    if (C == 1) return row[x];
    const u8 *p = row + 3 * x;
    return sv_gray_px(p[0], p[1], p[2]);
}

// gray of the 16 pixels x0..x0+15 of one row (only the first nvalid are read)
template <int C, bool VEC>
__device__ __forceinline__ void gray_row(const u8 *row, int x0, int nvalid, int (&g)[QP])
{
    if (VEC && nvalid == QP) {
        const u32x4 *p = reinterpret_cast<const u32x4 *>(row + C * x0);
        uint32_t w[4 * C];
#pragma unroll
        for (int k = 0; k < C; k++) {
            const u32x4 v = __builtin_nontemporal_load(p + k);
            w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
        }
#pragma unroll
        for (int i = 0; i < QP; i++) {
            if (C == 1) {
                g[i] = (w[i >> 2] >> (8 * (i & 3))) & 255;
            } else {
                int c[3];
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const int b = 3 * i + j;
                    c[j] = (w[b >> 2] >> (8 * (b & 3))) & 255;
                }
                g[i] = sv_gray_px(c[0], c[1], c[2]);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < QP; i++) g[i] = i < nvalid ? gray_at<C>(row, x0 + i) : 0;
    }
}

// Zeroes the three outputs the stats kernel accumulates into, one frame per workgroup.  A kernel and not hipMemsetAsync: captured
// into a graph, the two 8n-byte memsets zeroed the sums on the first replay only (tests/test_gpu_stream_order.py), and one launch
// replays like the stats kernel's own.
__global__ __launch_bounds__(256) void k_quality_clear(long long *__restrict__ lap_sum, long long *__restrict__ lap_sqsum, uint32_t *__restrict__ hist)
{
    hist[(ptrdiff_t)blockIdx.x * 256 + threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        lap_sum[blockIdx.x] = 0;
        lap_sqsum[blockIdx.x] = 0;
    }
}

template <int C, bool VEC>
__global__ __launch_bounds__(256) void k_frame_quality_stats(const u8 *__restrict__ img, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride,
                                                             int ntiles, int nsegs, long nitems, long long *__restrict__ lap_sum,
                                                             long long *__restrict__ lap_sqsum, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t sh[4][256 * QCOPIES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *h = sh[wave];
    for (int i = lane; i < 256 * QCOPIES; i += 64) h[i] = 0;
    __syncthreads();
    const long item = min((long)blockIdx.x * 4 + wave, nitems - 1);
    const bool active = (long)blockIdx.x * 4 + wave < nitems;   // the last block's spare waves only take part in the barriers
    const int per_frame = ntiles * nsegs;
    const int frame = (int)(item / per_frame);
    const int rem = (int)(item - (long)frame * per_frame);
    const int seg = rem / ntiles, tile = rem - seg * ntiles;
    const int x0 = tile * QTILE + lane * QP;
    const int nvalid = active ? sv_clamp(W - x0, 0, QP) : 0;
    const int y0 = seg * QROWS, y1 = active ? min(H, y0 + QROWS) : y0;
    const u8 *base = img + (ptrdiff_t)frame * img_stride;
    const int copy = lane % QCOPIES;

    int prev[QP], cur[QP], nxt[QP];
    gray_row<C, VEC>(base + (ptrdiff_t)sv_reflect101(y0 - 1, H) * pitch, x0, nvalid, prev);
    gray_row<C, VEC>(base + (ptrdiff_t)y0 * pitch, x0, nvalid, cur);
    long long s1 = 0, s2 = 0;
    for (int y = y0; y < y1; y++) {
        const u8 *row = base + (ptrdiff_t)y * pitch;
        gray_row<C, VEC>(base + (ptrdiff_t)sv_reflect101(y + 1, H) * pitch, x0, nvalid, nxt);
        // horizontal neighbours of the lane's first and last pixel: every lane shuffles, then the edge lanes read memory
        const int from_left = __shfl_up(cur[QP - 1], 1), from_right = __shfl_down(cur[0], 1);
        int L = from_left, R = from_right;
        if (nvalid > 0) {
            if (lane == 0) L = gray_at<C>(row, sv_reflect101(x0 - 1, W));
            if (lane == 63 || x0 + QP >= W) R = gray_at<C>(row, sv_reflect101(x0 + nvalid, W));
        }
        int r1 = 0, r2 = 0;                              // per row: |L| <= 1020, 16 px -> r2 < 2^25
#pragma unroll
        for (int i = 0; i < QP; i++) {
            if (i < nvalid) {
                const int left = i == 0 ? L : cur[i - 1];
                const int right = i + 1 < nvalid ? cur[i + 1] : R;
                const int lap = prev[i] + nxt[i] + left + right - 4 * cur[i];
                r1 += lap;
                r2 += lap * lap;
                atomicAdd(&h[cur[i] * QCOPIES + copy], 1u);
            }
        }
        s1 += r1;
        s2 += r2;
#pragma unroll
        for (int i = 0; i < QP; i++) { prev[i] = cur[i]; cur[i] = nxt[i]; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_down(s1, o);
        s2 += __shfl_down(s2, o);
    }
    __syncthreads();
    if (!active) return;
    if (lane == 0) {
        atomicAdd((unsigned long long *)&lap_sum[frame], (unsigned long long)s1);     // two's complement: the same bits as a signed add
        atomicAdd((unsigned long long *)&lap_sqsum[frame], (unsigned long long)s2);
    }
    uint32_t *gh = hist + (ptrdiff_t)frame * 256;
    for (int b = lane; b < 256; b += 64) {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < QCOPIES; k++) v += h[b * QCOPIES + k];
        if (v) atomicAdd(&gh[b], v);
    }
}

// compute_completeness's bands (cv/grid_quality.py:112-134): band 2i = rows, 2i+1 = columns [max(0,c-2), min(450,c+3)), c = min(50i, 449)
constexpr int QS = 450;

__device__ __forceinline__ int bit_tap(const uint32_t *bits, int H, int W, int x, int y)
{
    if ((unsigned)x >= (unsigned)W || (unsigned)y >= (unsigned)H) return 0;
    return ((bits[(ptrdiff_t)y * (W >> 5) + (x >> 5)] >> (x & 31)) & 1) * 255;
}

template <bool BITS>
__global__ __launch_bounds__(256) void k_grid_line_coverage(const void *__restrict__ src, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride,
                                                            const double *__restrict__ minv, uint32_t *__restrict__ counts)
{
    __shared__ double M[9];
    __shared__ uint32_t part[4];
    const int band = blockIdx.x, frame = blockIdx.y, tid = threadIdx.x;
    if (tid < 9) M[tid] = minv[frame * 9 + tid];
    __syncthreads();
    const int i = band >> 1;
    const bool vertical = band & 1;
    const int c = min(50 * i, QS - 1), lo = max(0, c - 2), hi = min(QS, c + 3), width = hi - lo;
    const int bw = sv_warp_block_w(QS, QS);
    uint32_t cnt = 0;
    for (int k = tid; k < width * QS; k += 256) {
        // k walks the band row-major in warped coordinates: rows of 450 (horizontal) or rows of `width` (vertical)
        int dx, dy;
        if (vertical) { dy = k / width; dx = lo + (k - dy * width); }
        else          { dy = lo + k / QS; dx = k - (dy - lo) * QS; }
        int sx, sy, a, b;
        sv_warp_coord(M, dx, dy, bw, sx, sy, a, b);
        int v;
        if (BITS) {
            const uint32_t *bits = (const uint32_t *)src + (ptrdiff_t)frame * H * (W >> 5);
            const int w00 = (32 - a) * (32 - b) * 32, w01 = a * (32 - b) * 32, w10 = (32 - a) * b * 32, w11 = a * b * 32;
            v = (bit_tap(bits, H, W, sx, sy) * w00 + bit_tap(bits, H, W, sx + 1, sy) * w01 + bit_tap(bits, H, W, sx, sy + 1) * w10 +
                 bit_tap(bits, H, W, sx + 1, sy + 1) * w11 + 16384) >> 15;
        } else {
            int px[1];
            sv_warp_sample<1>((const u8 *)src + (ptrdiff_t)frame * img_stride, H, W, pitch, sx, sy, a, b, px);
            v = px[0];
        }
        cnt += v > 0;
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
    if ((tid & 63) == 0) part[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) counts[frame * 20 + band] = part[0] + part[1] + part[2] + part[3];
}

}  // namespace

int svk_frame_quality_stats(const u8 *img, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int C, long long *lap_sum, long long *lap_sqsum,
                            uint32_t *hist, hipStream_t s)
{
    hipLaunchKernelGGL(k_quality_clear, dim3(n), dim3(256), 0, s, lap_sum, lap_sqsum, hist);
    SV_LAUNCH_CHECK("k_quality_clear");
    const int ntiles = (W + QTILE - 1) / QTILE, nsegs = (H + QROWS - 1) / QROWS;
    const long nitems = (long)n * ntiles * nsegs;
    const dim3 grid((unsigned)((nitems + 3) / 4));
    const bool vec = (((uintptr_t)img | (uintptr_t)pitch | (uintptr_t)img_stride) & 15) == 0;
    if (C == 3) {
        if (vec) hipLaunchKernelGGL((k_frame_quality_stats<3, true>), grid, dim3(256), 0, s, img, H, W, pitch, img_stride, ntiles, nsegs, nitems, lap_sum, lap_sqsum, hist);
        else     hipLaunchKernelGGL((k_frame_quality_stats<3, false>), grid, dim3(256), 0, s, img, H, W, pitch, img_stride, ntiles, nsegs, nitems, lap_sum, lap_sqsum, hist);
    } else {
        if (vec) hipLaunchKernelGGL((k_frame_quality_stats<1, true>), grid, dim3(256), 0, s, img, H, W, pitch, img_stride, ntiles, nsegs, nitems, lap_sum, lap_sqsum, hist);
        else     hipLaunchKernelGGL((k_frame_quality_stats<1, false>), grid, dim3(256), 0, s, img, H, W, pitch, img_stride, ntiles, nsegs, nitems, lap_sum, lap_sqsum, hist);
    }
    SV_LAUNCH_CHECK("k_frame_quality_stats");
    return SV_OK;
}

int svk_grid_line_coverage(const void *src, bool bits, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const double *minv, uint32_t *counts,
                           hipStream_t s)
{
    const dim3 grid(20, n);
    if (bits) hipLaunchKernelGGL(k_grid_line_coverage<true>, grid, dim3(256), 0, s, src, H, W, pitch, img_stride, minv, counts);
    else      hipLaunchKernelGGL(k_grid_line_coverage<false>, grid, dim3(256), 0, s, src, H, W, pitch, img_stride, minv, counts);
    SV_LAUNCH_CHECK("k_grid_line_coverage");
    return SV_OK;
}
