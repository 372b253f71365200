// Device half of the PNG decoder (cv2.imread of a .png after inflate): the filtered bytes of n images of one geometry -> BGR frames in HBM.  The host
// half (host_png.cpp) parses the container and inflates; sv_png_pixel.h has the arithmetic of one byte and one pixel.
//
// A row whose filter is None or Sub reads nothing from the row above, and neither does the image's first row: such a row starts a SEGMENT, which
// runs to the next such row.  Segments are independent.  Inside one, byte x of row r needs byte x - bpp of row r and bytes x, x - bpp of row r - 1.
//
//   k_png_rows      grid (ceil(H / 4), n), 256 threads: one WAVE per row.  A row that starts no segment leaves at once.  A segment of one None or
//                   Sub row -- every row of a file cv2 or our own encoder writes by default -- is finished here: Sub is a prefix sum per byte lane,
//                   64 pixels at a time, the bpp byte lanes of a pixel packed in one 64-bit word and added without carries between them.  Any other
//                   segment's first row is appended to the job list (one atomic add per segment).
//   k_png_segments  grid (at most 4 per CU), 64 threads: one wave per segment, jobs taken blockIdx.x, + gridDim.x, ...  Rows go in stripes of
//                   kStripe = 64 (lane = row), a stripe in chunks of kChunk = 512 bytes staged in LDS.  Inside a chunk the rows form a skewed
//                   wavefront, row r one byte behind row r - 1: in step s lane l does byte s - l, takes `above` from lane l - 1's last result by
//                   one cross-lane move (lane 0: from the LDS copy of the row above the stripe) and keeps the last 8 bytes of its own row and of
//                   the row above in two 64-bit registers, so `left` and `above-left` are shifts.  A chunk costs its bytes + 63 steps.
//   k_png_expand    grid (ceil(W / 256), H, n): one thread per pixel, unfiltered samples -> B, G, R.
//   k_png_expand_gray   the same grid, one gray byte a pixel (svpng::expand_gray): the IMREAD_GRAYSCALE read, in k_png_expand's place.
//
// No wave waits for another: the job list is complete at the launch boundary, k_png_segments never looks at a row another workgroup writes
// (a segment's first row needs nothing from above), and every loop is bounded by the geometry.  The scratch (ctx->png_dec) is
//   u8 raw[n][H][row_bytes] | pad to 16 | u32 count, pad[3] | u32 jobs[n * H]      (a job = image * H + first row)
#include "sv_internal.h"
#include "sv_png_pixel.h"

namespace {

constexpr int kStripe = 64, kChunk = 512;
constexpr int kPitch = kChunk + 5;                 // (kPitch - 1) / 4 is odd: the skewed wave's 64 byte addresses fall into distinct banks

struct DecGeom {
    int W, H, bpp, color_type, bit_depth, channels;
    long row_bytes, filtered_bytes;
};

__device__ inline unsigned filter_of(const u8 *rf, int r)
{
    const unsigned f = rf[r];
    return f > 4 ? 0u : f;
}

// byte lanes added modulo 256 each
__device__ inline uint64_t add_bytes(uint64_t x, uint64_t y)
{
    const uint64_t low = 0x7f7f7f7f7f7f7f7full;
    return ((x & low) + (y & low)) ^ ((x ^ y) & ~low);
}

// Zeroes the job counter and the per-image status.  A kernel and not hipMemsetAsync: captured into a graph, a 16-byte memset zeroed
// its target on the first replay only (seen on K6's sums, tests/test_gpu_stream_order.py), and a job counter that is not zero
// sends k_png_rows' jobs[atomicAdd(count, 1)] past the scratch.
__global__ __launch_bounds__(256) void k_png_clear(uint32_t *__restrict__ count, uint32_t *__restrict__ status, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *count = 0;
    if (i < n) status[i] = 0;
}

__global__ __launch_bounds__(256) void k_png_rows(const u8 *__restrict__ filtered, const u8 *__restrict__ row_filter, DecGeom g, u8 *__restrict__ raw,
                                                  uint32_t *__restrict__ count, uint32_t *__restrict__ jobs)
{
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6), img = blockIdx.y;
    if (r >= g.H) return;
    const u8 *rf = row_filter + (long)img * g.H;
    unsigned f = filter_of(rf, r);
    if (r > 0 && f > 1) return;                                        // inside a segment
    if (r == 0) f = f == 2 ? 0u : f == 4 ? 1u : f;                     // nothing above: Up is None, Paeth is Sub
    const bool single = r + 1 == g.H || filter_of(rf, r + 1) <= 1;
    if (!single || f > 1) {
        if (lane == 0) jobs[atomicAdd(count, 1u)] = (uint32_t)img * (uint32_t)g.H + (uint32_t)r;
        return;
    }
    const u8 *src = filtered + (long)img * g.filtered_bytes + (long)r * (1 + g.row_bytes) + 1;
    u8 *dst = raw + ((long)img * g.H + r) * g.row_bytes;
    if (f == 0) {
        for (long i = lane; i < g.row_bytes; i += 64) dst[i] = src[i];
        return;
    }
    const long npix = g.row_bytes / g.bpp;                             // row_bytes is a multiple of bpp
    uint64_t carry = 0;
    for (long base = 0; base < npix; base += 64) {
        const long px = base + lane;
        uint64_t v = 0;
        if (px < npix)
            for (int k = 0; k < g.bpp; k++) v |= (uint64_t)src[px * g.bpp + k] << (8 * k);
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t t = __shfl_up(v, d);
            if (lane >= d) v = add_bytes(v, t);
        }
        v = add_bytes(v, carry);
        if (px < npix)
            for (int k = 0; k < g.bpp; k++) dst[px * g.bpp + k] = (u8)(v >> (8 * k));
        carry = __shfl(v, 63);
    }
}

__global__ __launch_bounds__(64) void k_png_segments(const u8 *__restrict__ filtered, const u8 *__restrict__ row_filter, DecGeom g, u8 *raw,
                                                     const uint32_t *__restrict__ count, const uint32_t *__restrict__ jobs)
{
    __shared__ u8 tile[(kStripe + 1) * kPitch];                        // row 0: the row above the stripe
    const int lane = threadIdx.x;
    const uint32_t njobs = *count;
    for (uint32_t job = blockIdx.x; job < njobs; job += gridDim.x) {
        const int img = (int)(jobs[job] / (uint32_t)g.H), r0 = (int)(jobs[job] % (uint32_t)g.H);
        const u8 *rf = row_filter + (long)img * g.H;
        const u8 *fimg = filtered + (long)img * g.filtered_bytes;
        u8 *rimg = raw + (long)img * g.H * g.row_bytes;
        int r1 = g.H;                                                  // the next segment's first row
        for (int base = r0 + 1; base < g.H; base += 64) {
            const int rr = base + lane;
            const unsigned long long starts = __ballot(rr >= g.H || filter_of(rf, rr) <= 1);
            if (starts) { r1 = base + __ffsll(starts) - 1; break; }
        }
        for (int s0 = r0; s0 < r1; s0 += kStripe) {
            const int rows = min(kStripe, r1 - s0);
            const bool active = lane < rows;
            const unsigned f = active ? filter_of(rf, s0 + lane) : 0u;
            uint64_t mine = 0, above = 0;                              // the last 8 bytes of this row and of the row above it, newest lowest
            const int back = 8 * (g.bpp - 1);
            for (long c0 = 0; c0 < g.row_bytes; c0 += kChunk) {
                const int cb = (int)min((long)kChunk, g.row_bytes - c0);
                for (int i = lane; i < cb; i += 64) tile[i] = s0 == r0 ? (u8)0 : rimg[(long)(s0 - 1) * g.row_bytes + c0 + i];
                for (int rr = 0; rr < rows; rr++)
                    for (int i = lane; i < cb; i += 64) tile[(rr + 1) * kPitch + i] = fimg[(long)(s0 + rr) * (1 + g.row_bytes) + 1 + c0 + i];
                __syncthreads();
                u8 *own = tile + (lane + 1) * kPitch;
                for (int s = 0; s < cb + rows - 1; s++) {
                    const int x = s - lane;
                    const unsigned handed = __shfl_up((unsigned)(mine & 255u), 1);
                    if (active && x >= 0 && x < cb) {
                        const unsigned b = lane == 0 ? tile[x] : handed;
                        const unsigned v = svpng::unfilter_byte(f, own[x], (unsigned)(mine >> back) & 255u, b, (unsigned)(above >> back) & 255u);
                        mine = mine << 8 | v;
                        above = above << 8 | b;
                        own[x] = (u8)v;
                    }
                }
                __syncthreads();
                for (int rr = 0; rr < rows; rr++)
                    for (int i = lane; i < cb; i += 64) rimg[(long)(s0 + rr) * g.row_bytes + c0 + i] = tile[(rr + 1) * kPitch + i];
                __syncthreads();
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_png_expand(const u8 *__restrict__ raw, const u8 *__restrict__ palette, DecGeom g, u8 *__restrict__ out, long pitch,
                                                    long frame_stride, uint32_t *__restrict__ status)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, img = blockIdx.z;
    if (x >= g.W) return;
    const u8 *pal = palette ? palette + (long)img * SV_PNG_PALETTE_STRIDE : nullptr;
    const unsigned pal_n = pal ? min(256u, *(const uint32_t *)(pal + 768)) : 0u;
    const svpng::Expand e = {g.color_type, g.bit_depth, g.channels};
    const uint32_t px = svpng::expand_pixel(e, raw + ((long)img * g.H + y) * g.row_bytes, x, pal, pal_n);
    if (px >> 24) atomicOr(status + img, 1u);
    u8 *o = out + (long)img * frame_stride + (long)y * pitch + 3L * x;
    o[0] = (u8)px; o[1] = (u8)(px >> 8); o[2] = (u8)(px >> 16);
}

__global__ __launch_bounds__(256) void k_png_expand_gray(const u8 *__restrict__ raw, const u8 *__restrict__ palette, DecGeom g, u8 *__restrict__ out, long pitch,
                                                         long frame_stride, uint32_t *__restrict__ status)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, img = blockIdx.z;
    if (x >= g.W) return;
    const u8 *pal = palette ? palette + (long)img * SV_PNG_PALETTE_STRIDE : nullptr;
    const unsigned pal_n = pal ? min(256u, *(const uint32_t *)(pal + 768)) : 0u;
    const svpng::Expand e = {g.color_type, g.bit_depth, g.channels};
    const unsigned px = svpng::expand_gray(e, raw + ((long)img * g.H + y) * g.row_bytes, x, pal, pal_n);
    if (px >> 8) atomicOr(status + img, 1u);
    out[(long)img * frame_stride + (long)y * pitch + x] = (u8)px;
}

}  // namespace

int svk_png_reconstruct(sv_ctx *ctx, const sv_png_info *info, const u8 *filtered, const u8 *row_filter, const u8 *palette, int n, u8 *out, ptrdiff_t pitch,
                        ptrdiff_t frame_stride, uint32_t *status, bool gray, hipStream_t s)
{
    DecGeom g = {};
    g.W = info->width; g.H = info->height; g.bpp = info->bpp; g.color_type = info->color_type; g.bit_depth = info->bit_depth; g.channels = info->channels;
    g.row_bytes = info->row_bytes; g.filtered_bytes = info->filtered_bytes;
    const size_t raw_bytes = ((size_t)n * (size_t)g.H * (size_t)g.row_bytes + 15) / 16 * 16, rows = (size_t)n * (size_t)g.H;
    const int rc = ctx->png_dec.grow(ctx, raw_bytes + 16 + 4 * rows);
    if (rc) return rc;
    u8 *raw = ctx->png_dec.as<u8>();
    uint32_t *count = (uint32_t *)(raw + raw_bytes), *jobs = count + 4;
    hipLaunchKernelGGL(k_png_clear, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, count, status, n);
    SV_LAUNCH_CHECK("k_png_clear");
    hipLaunchKernelGGL(k_png_rows, dim3((unsigned)((g.H + 3) / 4), (unsigned)n), dim3(256), 0, s, filtered, row_filter, g, raw, count, jobs);
    SV_LAUNCH_CHECK("k_png_rows");
    const unsigned grid = (unsigned)std::min<size_t>(rows, (size_t)ctx->num_cus * 4);
    hipLaunchKernelGGL(k_png_segments, dim3(grid), dim3(64), 0, s, filtered, row_filter, g, raw, (const uint32_t *)count, (const uint32_t *)jobs);
    SV_LAUNCH_CHECK("k_png_segments");
    hipLaunchKernelGGL(gray ? k_png_expand_gray : k_png_expand, dim3((unsigned)((g.W + 255) / 256), (unsigned)g.H, (unsigned)n), dim3(256), 0, s, (const u8 *)raw, palette, g,
                       out, (long)pitch, (long)frame_stride, status);
    SV_LAUNCH_CHECK(gray ? "k_png_expand_gray" : "k_png_expand");
    return SV_OK;
}
