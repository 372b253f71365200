// Device half of the PNG encoder (cv2.imwrite(path.png) with cv2's defaults: the Sub filter on every row, Z_BEST_SPEED, Z_RLE): BGR or gray frames in
// HBM -> the deflate stream of the filtered image, cut into bands of whole rows that are compressed independently (sv_png_band.h has the band's
// algorithm, phase by phase, and the format of its piece of the stream).  The host half (host_png.cpp) wraps the stream into the file.
//
//   k_png_band      grid (bands, n), 256 threads: one workgroup per band of one frame, everything in LDS (the filtered band, the packed block, the
//                   histogram and the Huffman tree: 80 KB for bands up to 35,000 bytes, two workgroups a CU; 140 KB for bands up to 65,535 bytes).
//                   No workgroup waits for another; every loop is bounded by the band's byte count or by a constant.  The band's bytes go to its
//                   slot in the context's png_enc scratch (slot = the stored band + 10, rounded up to 16), its length, Adler-32 and status out.
//   k_png_compact   grid (bands, n): the band's offset in the frame's stream = the sum of the lengths before it; copies the slot there.
// Only the compact stream and the lengths cross PCIe.
#include "sv_internal.h"
#include "sv_png_band.h"

namespace {

using namespace svpng;

template <int CAP>
__global__ __launch_bounds__(kThreads) void k_png_band(const u8 *__restrict__ src, Geom g, u8 *__restrict__ slots, uint32_t *__restrict__ band_len,
                                                       uint32_t *__restrict__ adler, uint32_t *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) Band<CAP> b;
    const int tid = threadIdx.x, band = blockIdx.x, frame = blockIdx.y;
    const u8 *img = src + (long)frame * g.frame_stride;
    const long at = (long)frame * g.bands + band;
    Lane L;
    b.p0_init(g, band, tid);
    __syncthreads();
    if (g.filter == kFilterAdaptive) {
        b.p1_row_sums(g, img, tid);
        __syncthreads();
        b.p2_row_choice(tid);
        __syncthreads();
    }
    b.p3_filter(g, img, tid);
    __syncthreads();
    b.p4_chunks(tid);
    __syncthreads();
    b.p5_histogram(g, L, tid);
    __syncthreads();
    if (g.strategy != kStored) {
        b.p6_keys(tid);
        __syncthreads();
        b.p7_rank(tid);
        __syncthreads();
        b.p8_code(tid);
        __syncthreads();
        b.p9_measure(g, L, tid);
        __syncthreads();
    }
    b.p10_pack(g, L, tid);
    __syncthreads();
    b.p11_store(g, slots + at * g.slot_bytes, band_len + at, adler + at, status + at, tid);
}

__global__ __launch_bounds__(kThreads) void k_png_compact(const u8 *__restrict__ slots, const uint32_t *__restrict__ band_len, int bands, long slot_bytes,
                                                          long stream_bound, u8 *__restrict__ stream)
{
    __shared__ unsigned long long before;
    const int tid = threadIdx.x, band = blockIdx.x, frame = blockIdx.y;
    const uint32_t *len = band_len + (long)frame * bands;
    if (tid == 0) before = 0;
    __syncthreads();
    unsigned long long s = 0;
    for (int j = tid; j < band; j += kThreads) s += len[j];
    if (s) atomicAdd(&before, s);
    __syncthreads();
    const long off = (long)before, n = len[band];
    if (off + n > stream_bound) return;                                // cannot happen: every length is at most its slot's share of the bound
    const u8 *from = slots + ((long)frame * bands + band) * slot_bytes;
    u8 *to = stream + (long)frame * stream_bound + off;
    for (long i = tid; i < n; i += kThreads) to[i] = from[i];
}

}  // namespace

int svk_png_deflate(sv_ctx *ctx, const sv_png_enc *plan, const u8 *src, int n, ptrdiff_t pitch, ptrdiff_t frame_stride, u8 *stream, uint32_t *band_len, uint32_t *adler,
                    uint32_t *status, hipStream_t s)
{
    Geom g = {};
    g.W = plan->width; g.H = plan->height; g.bpp = plan->channels;
    g.filter = plan->filter; g.strategy = plan->strategy;
    g.band_rows = plan->band_rows; g.bands = plan->bands; g.row_bytes = (int)plan->row_bytes;
    g.pitch = (long)pitch; g.frame_stride = (long)frame_stride; g.slot_bytes = plan->slot_bytes;
    const int rc = ctx->png_enc.grow(ctx, (size_t)n * (size_t)plan->bands * (size_t)plan->slot_bytes);
    if (rc) return rc;
    u8 *slots = ctx->png_enc.as<u8>();
    const dim3 grid((unsigned)plan->bands, (unsigned)n);
    if ((long)plan->band_rows * plan->row_bytes <= kSmallBandBytes)
        hipLaunchKernelGGL(k_png_band<kSmallBandBytes>, grid, dim3(kThreads), 0, s, src, g, slots, band_len, adler, status);
    else
        hipLaunchKernelGGL(k_png_band<kMaxBandBytes>, grid, dim3(kThreads), 0, s, src, g, slots, band_len, adler, status);
    SV_LAUNCH_CHECK("k_png_band");
    hipLaunchKernelGGL(k_png_compact, grid, dim3(kThreads), 0, s, (const u8 *)slots, (const uint32_t *)band_len, plan->bands, (long)plan->slot_bytes, (long)plan->stream_bound,
                       stream);
    SV_LAUNCH_CHECK("k_png_compact");
    return SV_OK;
}
