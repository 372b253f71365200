// K20: the luma-only JPEG decode -- cv2.imread(path, cv2.IMREAD_GRAYSCALE / IMREAD_REDUCED_GRAYSCALE_2 / _4 / _8) for JPEG files
// (ml/datasets.py:81,153, ml/evaluate.py:67, tools/augment_data.py:328,361, tools/dataset_stats.py:211,245, tools/label_cells.py:42).
// libjpeg with out_color_space = JCS_GRAYSCALE returns the inverse DCT of the Y component and never touches Cb or Cr; so does this:
// Y-only coefficient records (host_jpeg.cpp's luma mode) -> the uint8 [H, W] image in the caller's buffer.  No component planes, no
// colour kernel: one launch.
//
// The transforms are the colour path's (sv_jpeg_idct.h), at scale 1 / d a block comes out at S = 8 / d samples per side.  New here:
//   front  Y records lie in SCAN order -- MCU after MCU, the 2x2 (4:2:0) or 2x1 (4:2:2) luma blocks of an MCU row-major -- so the record of
//          the block at raster position (bx, by) is ((by / v) * mcu_cols + bx / h) * h * v + (by % v) * h + bx % h, computed per block.
//          Only blocks that intersect the image are transformed; the MCU padding is never read.
//   back   a workgroup takes horizontally adjacent blocks of one block row, and a store instruction's lanes run along image rows:
//          S = 8   32 blocks; the samples go through an LDS tile of 8 rows x 256 bytes, then thread t stores 8 bytes of row t / 32 at
//                  column 8 * (t % 32): a wavefront writes 2 rows of 256 contiguous bytes
//          S = 4   64 blocks; LDS tile of 4 rows x 256 bytes, thread t stores 4 bytes of row t / 64: a wavefront writes 256 contiguous bytes
//          S = 2   a wavefront takes 64 adjacent blocks in registers, two 2-byte stores per lane: 128 contiguous bytes per row
//          S = 1   a wavefront takes 64 adjacent blocks, one byte per lane
//          Rows are clipped at the image's right and bottom edges; a row start or pitch that breaks the store's alignment, a clipped run and
//          an EXIF orientation other than 1 (a rotated or mirrored destination) go byte by byte.
#include "sv_internal.h"
#include "sv_jpeg_idct.h"

namespace {

struct JpegGrayGeom {
    int W, H;                          // the decoded image as stored: ceil(width / d) x ceil(height / d)
    int orientation;
    int bwi, bhi;                      // blocks that intersect the image
    int mcu_cols, hsh, vsh;            // MCUs per row; log2 of luma's sampling factors
};

__device__ __forceinline__ long luma_record(const JpegGrayGeom &g, int bx, int by)
{
    const int hm = (1 << g.hsh) - 1, vm = (1 << g.vsh) - 1;
    return ((((long)(by >> g.vsh) * g.mcu_cols + (bx >> g.hsh)) << (g.hsh + g.vsh)) + ((by & vm) << g.hsh)) + (bx & hm);
}

// where sample (x, y) of the stored W x H image lies in the output under the EXIF orientation (the inverse of k5_jpeg.hip's source_xy)
__device__ __forceinline__ void dest_xy(int orientation, int W, int H, int x, int y, int &ox, int &oy)
{
    switch (orientation) {
    case 2: ox = W - 1 - x; oy = y; break;
    case 3: ox = W - 1 - x; oy = H - 1 - y; break;
    case 4: ox = x; oy = H - 1 - y; break;
    case 5: ox = y; oy = x; break;
    case 6: ox = H - 1 - y; oy = x; break;
    case 7: ox = H - 1 - y; oy = W - 1 - x; break;
    case 8: ox = y; oy = W - 1 - x; break;
    default: ox = x; oy = y;
    }
}

// N samples (low byte first) of stored row y from column x on, clipped to the image
template <int N>
__device__ __forceinline__ void store_samples(u8 *__restrict__ out, long pitch, const JpegGrayGeom &g, int x, int y, unsigned long long px)
{
    if (y >= g.H || x >= g.W) return;
    if (g.orientation == 1) {
        u8 *p = out + (long)y * pitch + x;
        if (x + N <= g.W && ((uintptr_t)p & (N - 1)) == 0) {
            if (N == 8) *(uint2 *)p = make_uint2((unsigned)px, (unsigned)(px >> 32));
            else if (N == 4) *(unsigned *)p = (unsigned)px;
            else if (N == 2) *(unsigned short *)p = (unsigned short)px;
            else *p = (u8)px;
        } else {
#pragma unroll
            for (int i = 0; i < N; i++)
                if (x + i < g.W) p[i] = (u8)(px >> (8 * i));
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
        if (x + i >= g.W) break;
        int ox, oy;
        dest_xy(g.orientation, g.W, g.H, x + i, y, ox, oy);
        out[(long)oy * pitch + ox] = (u8)(px >> (8 * i));
    }
}

template <bool SPARSE>
__global__ __launch_bounds__(256) void k_jpeg_gray8(const short *__restrict__ coef, const unsigned long long *__restrict__ masks,
                                                     const unsigned *__restrict__ offsets, const short *__restrict__ values,
                                                     const unsigned short *__restrict__ quant, JpegGrayGeom g, u8 *__restrict__ out, long pitch)
{
    __shared__ int ws[32][8][9];
    __shared__ __align__(8) unsigned tile[8][72];               // [row][word], rows padded by 8 words
    const int tid = threadIdx.x, b = tid >> 3, r = tid & 7;
    const int bx = blockIdx.x * 32 + b, by = blockIdx.y;
    const bool live = bx < g.bwi;
    const long rec = live ? luma_record(g, bx, by) : 0;
    unsigned lo, hi;
    jpeg_idct8_row<SPARSE>(ws, b, r, live, SPARSE ? nullptr : coef + rec * 64, SPARSE && live ? masks[rec] : 0, SPARSE && live ? values + offsets[rec] : nullptr,
                           quant, lo, hi);
    *(uint2 *)&tile[r][2 * b] = make_uint2(lo, hi);
    __syncthreads();
    const int row = tid >> 5, k = tid & 31;
    const uint2 v = *(const uint2 *)&tile[row][2 * k];
    store_samples<8>(out, pitch, g, (blockIdx.x * 32 + k) * 8, by * 8 + row, (unsigned long long)v.y << 32 | v.x);
}

template <bool SPARSE>
__global__ __launch_bounds__(256) void k_jpeg_gray4(const short *__restrict__ coef, const unsigned long long *__restrict__ masks,
                                                     const unsigned *__restrict__ offsets, const short *__restrict__ values,
                                                     const unsigned short *__restrict__ quant, JpegGrayGeom g, u8 *__restrict__ out, long pitch)
{
    __shared__ int ws[64][73];
    __shared__ unsigned tile[4][72];                            // [row][block]; 72: rows start 8 banks apart, a 32-lane group's writes do not collide
    const int tid = threadIdx.x, b = tid >> 2, t = tid & 3;
    const int bx = blockIdx.x * 64 + b, by = blockIdx.y;
    const bool live = bx < g.bwi;
    const long rec = live ? luma_record(g, bx, by) : 0;
    tile[t][b] = jpeg_idct4_row<SPARSE>(ws, b, t, live, SPARSE ? nullptr : coef + rec * 64, SPARSE && live ? masks[rec] : 0,
                                        SPARSE && live ? values + offsets[rec] : nullptr, quant);
    __syncthreads();
    const int row = tid >> 6, k = tid & 63;
    store_samples<4>(out, pitch, g, (blockIdx.x * 64 + k) * 4, by * 4 + row, tile[row][k]);
}

// S = 2, 1: a wavefront per run of 64 adjacent blocks, four block rows per workgroup
template <int S, bool SPARSE>
__global__ __launch_bounds__(256) void k_jpeg_gray_small(const short *__restrict__ coef, const unsigned long long *__restrict__ masks,
                                                          const unsigned *__restrict__ offsets, const short *__restrict__ values,
                                                          const unsigned short *__restrict__ quant, JpegGrayGeom g, u8 *__restrict__ out, long pitch)
{
    static_assert(S == 1 || S == 2, "block sizes 1 and 2");
    const int bx = blockIdx.x * 64 + (threadIdx.x & 63), by = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (bx >= g.bwi || by >= g.bhi) return;
    const long rec = luma_record(g, bx, by);
    const short *blk = SPARSE ? nullptr : coef + rec * 64;
    const unsigned long long mask = SPARSE ? masks[rec] : 0;
    const short *vals = SPARSE ? values + offsets[rec] : nullptr;
    if (S == 1) store_samples<1>(out, pitch, g, bx, by, jpeg_idct1_block<SPARSE>(blk, mask, vals, quant));
    else {
        unsigned top = 0, bottom = 0;
        jpeg_idct2_block<SPARSE>(blk, mask, vals, quant, 0, top, bottom);
        store_samples<2>(out, pitch, g, 2 * bx, 2 * by, top);
        store_samples<2>(out, pitch, g, 2 * bx, 2 * by + 1, bottom);
    }
}

using GrayKernel = void (*)(const short *, const unsigned long long *, const unsigned *, const short *, const unsigned short *, JpegGrayGeom, u8 *, long);

template <bool SPARSE>
constexpr GrayKernel gray_kernel(int S)
{
    return S == 8 ? k_jpeg_gray8<SPARSE> : S == 4 ? k_jpeg_gray4<SPARSE> : S == 2 ? k_jpeg_gray_small<2, SPARSE> : k_jpeg_gray_small<1, SPARSE>;
}

}  // namespace

// info: what sv_jpeg_parse_luma reports (coef_count counts Y's blocks alone); gray: ceil(out_height / denom) x ceil(out_width / denom)
int svk_jpeg_reconstruct_gray(const sv_jpeg_info *info, int denom, const int16_t *coef, const uint64_t *masks, const uint32_t *offsets, const int16_t *values,
                              const uint16_t *quant, u8 *gray, ptrdiff_t pitch, hipStream_t s, const char *fn)
{
    const int hs = info->h_samp, vs = info->v_samp, S = 8 / denom;
    const int mcu_cols = (info->width + 8 * hs - 1) / (8 * hs), mcu_rows = (info->height + 8 * vs - 1) / (8 * vs);
    const long want = 64L * mcu_cols * mcu_rows * hs * vs;
    if (want != info->coef_count) return sv_fail(SV_ERR_BAD_ARG, "%s: coef_count %ld is not the luma block count of the geometry (%ld)", fn, info->coef_count, want);
    JpegGrayGeom g = {};
    g.W = (info->width + denom - 1) / denom; g.H = (info->height + denom - 1) / denom;
    g.orientation = info->orientation;
    g.bwi = (g.W + S - 1) / S; g.bhi = (g.H + S - 1) / S;       // = ceil(width / 8), ceil(height / 8): within the MCU grid
    g.mcu_cols = mcu_cols; g.hsh = hs - 1; g.vsh = vs - 1;
    const int per_x = S == 8 ? 32 : 64, per_y = S >= 4 ? 1 : 4;
    const GrayKernel k = coef ? gray_kernel<false>(S) : gray_kernel<true>(S);
    hipLaunchKernelGGL(k, dim3((unsigned)((g.bwi + per_x - 1) / per_x), (unsigned)((g.bhi + per_y - 1) / per_y)), dim3(256), 0, s, (const short *)coef,
                       (const unsigned long long *)masks, offsets, (const short *)values, quant, g, gray, (long)pitch);
    SV_LAUNCH_CHECK("k_jpeg_gray");
    return SV_OK;
}
