// Device half of the JPEG encoder (cv2.imwrite at pipeline/run.py:431): BGR or gray frames in HBM -> quantised coefficient blocks, dense and in the
// sparse transport form of the decoder (host_jpeg.cpp: per block a 64-bit mask over ZIGZAG positions and the index of its first value, the non-zero
// values in zigzag order).  The serial Huffman bit packing stays on the host (host_jpeg.cpp).  Integer arithmetic throughout, bit-exact with
// libjpeg-turbo's defaults: rgb_ycc fixed-point colour conversion, h2v1 / h2v2 down-sampling with the alternating bias, edge replication, the
// JDCT_ISLOW forward DCT (jfdctint.c) and a quantiser that divides by 8 q rounding half away from zero.
//
//   k_jpeg_forward   one workgroup per tile of 128 pixels x one MCU row (8 or 16 pixel rows; 16 or 8 MCUs) of one frame.
//                    1. every thread converts pixels, consecutive threads consecutive pixels of a row (the frame is read once, coordinates clamped
//                       to the image: that is libjpeg's right / bottom edge replication of the full-size rows; at 4:2:0 the chroma rows below
//                       the image repeat the last down-sampled row instead, so they take that row's two source rows), into full-size
//                       Y, Cb, Cr byte planes in LDS;
//                    2. eight threads per block: thread r takes sample row r (chroma rows are down-sampled here, from the LDS planes), runs the
//                       row pass in registers and writes it to an LDS workspace (rows padded to 9 words);
//                    3. the same thread runs the column pass on column r and quantises it in place: |x| + 4 q times ceil(2^32 / 8 q), high word --
//                       exact for every dividend below 2^21, the FDCT's outputs are below 2^16;
//                    4. dummy blocks (those of an MCU beyond the component's own block grid; luma at 4:2:2 / 4:2:0 only) get zero AC and the DC
//                       of the block before them in the MCU (jccoefct.c): they change no decoded pixel, but they are in the file;
//                    5. thread r stores natural-order row r of the block (16 bytes), and builds the byte of the mask for zigzag positions
//                       8 r .. 8 r + 7; thread 0 of the block stores the mask and its popcount.
//   k_jpeg_scan      one workgroup per frame: exclusive prefix sum of the popcounts, in place -> offsets; the frame's total -> counts[frame].
//   k_jpeg_compact   eight threads per block: thread r writes the non-zero values of zigzag positions 8 r .. 8 r + 7 at offsets[block] + rank.
// Scratch: the dense blocks, when the caller does not ask for them, live in the context's grow-only jpeg_enc buffer.  A tile's 48 blocks at most
// and 6 KB of planes keep a workgroup at 20 KB of LDS; the transforms never leave registers and LDS.
#include "sv_internal.h"

namespace {

struct JpegEncGeom {
    int W, H, ncomp, hs, vs;           // luma sampling factors; chroma is 1x1
    int mcu_cols;
    int bw[3], own_bw[3], own_bh[3];   // block grid over whole MCUs; the component's own grid (the rest are dummy blocks)
    long block_off[3];                 // first block of each component
    long nblocks;                      // per frame
    unsigned short quant[192];         // natural order, per component
    unsigned recip[192];               // ceil(2^32 / (8 q))
};

// zigzag index -> natural (row-major) position
__constant__ unsigned char kNaturalOf[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 8-point pass of jfdctint.c (CONST_BITS 13, PASS1_BITS 2)
template <bool FIRST>
__device__ __forceinline__ void fdct8(const int (&d)[8], int (&o)[8])
{
    constexpr int N = FIRST ? 11 : 15;
    int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    o[0] = FIRST ? (tmp10 + tmp11) * 4 : descale(tmp10 + tmp11, 2);
    o[4] = FIRST ? (tmp10 - tmp11) * 4 : descale(tmp10 - tmp11, 2);
    int z1 = (tmp12 + tmp13) * 4433;
    o[2] = descale(z1 + tmp13 * 6270, N);
    o[6] = descale(z1 + tmp12 * (-15137), N);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    tmp4 *= 2446; tmp5 *= 16819; tmp6 *= 25172; tmp7 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    o[7] = descale(tmp4 + z1 + z3, N);
    o[5] = descale(tmp5 + z2 + z4, N);
    o[3] = descale(tmp6 + z2 + z3, N);
    o[1] = descale(tmp7 + z1 + z4, N);
}

constexpr int kTileW = 128;            // pixels per tile row: 16 MCUs of 8, or 8 of 16
constexpr int kMaxBlocks = 48;         // 4:4:4: 3 x 16; 4:2:0: 2 x 16 + 2 x 8

// Block b of a tile: its component, block row within the MCU row and block column within the tile.  Luma first (vs rows of 16), then Cb, then Cr.
__device__ __forceinline__ void tile_block(const JpegEncGeom &g, int b, int &c, int &byl, int &bxl)
{
    const int ny = 16 * g.vs, nc = kTileW / (8 * g.hs);
    if (b < ny) { c = 0; byl = b >> 4; bxl = b & 15; }
    else { c = 1 + (b - ny) / nc; byl = 0; bxl = (b - ny) % nc; }
}

template <int CH>
__global__ __launch_bounds__(256) void k_jpeg_forward(const u8 *__restrict__ src, long pitch, long img_stride, JpegEncGeom g, short *__restrict__ coef,
                                                       unsigned long long *__restrict__ masks, unsigned *__restrict__ offsets)
{
    __shared__ u8 samp[3][16 * kTileW];
    __shared__ int ws[kMaxBlocks][8][9];
    __shared__ __attribute__((aligned(8))) u8 mbyte[kMaxBlocks][8];
    const int tid = threadIdx.x, frame = blockIdx.z, my = blockIdx.y, tile = blockIdx.x;
    const int mh = 8 * g.vs, x0 = tile * kTileW, y0 = my * mh;
    const u8 *img = src + (long)frame * img_stride;
    // 1. colour conversion (jccolor.c rgb_ycc_convert on BGR input); clamped coordinates replicate the right and bottom edges
    for (int i = tid; i < mh * kTileW; i += 256) {
        const int ty = i >> 7, tx = i & (kTileW - 1);
        const int x = min(x0 + tx, g.W - 1), y = min(y0 + ty, g.H - 1);
        const u8 *px = img + (long)y * pitch + (long)x * CH;
        if (CH == 1) samp[0][i] = px[0];
        else {
            int B = px[0], G = px[1], R = px[2];
            samp[0][i] = (u8)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
            if (g.vs == 2) {
                // below the image libjpeg repeats the last DOWN-SAMPLED chroma row (jcprepct.c pads the colour rows to a row group only): the two
                // source rows of that row, not the last image row twice
                const int crow = min((y0 + ty) >> 1, (g.H + 1) / 2 - 1), yc = min(2 * crow + (ty & 1), g.H - 1);
                if (yc != y) {
                    px = img + (long)yc * pitch + (long)x * CH;
                    B = px[0]; G = px[1]; R = px[2];
                }
            }
            samp[1][i] = (u8)((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16);
            samp[2][i] = (u8)((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16);
        }
    }
    __syncthreads();
    const int nblk = CH == 1 ? 16 : 16 * g.vs + 2 * (kTileW / (8 * g.hs));
    // 2. row pass
    for (int t = tid; t < nblk * 8; t += 256) {
        const int b = t >> 3, r = t & 7;
        int c, byl, bxl;
        tile_block(g, b, c, byl, bxl);
        int d[8], o[8];
        if (c == 0 || g.hs == 1) {
            const u8 *p = &samp[c][(byl * 8 + r) * kTileW + bxl * 8];
#pragma unroll
            for (int i = 0; i < 8; i++) d[i] = (int)p[i] - 128;
        } else if (g.vs == 1) {                                        // h2v1_downsample: bias 0, 1, 0, 1, ...
            const u8 *p = &samp[c][r * kTileW + bxl * 16];
#pragma unroll
            for (int i = 0; i < 8; i++) d[i] = ((p[2 * i] + p[2 * i + 1] + (i & 1)) >> 1) - 128;
        } else {                                                       // h2v2_downsample: bias 1, 2, 1, 2, ...
            const u8 *p = &samp[c][2 * r * kTileW + bxl * 16];
#pragma unroll
            for (int i = 0; i < 8; i++) d[i] = ((p[2 * i] + p[2 * i + 1] + p[kTileW + 2 * i] + p[kTileW + 2 * i + 1] + 1 + (i & 1)) >> 2) - 128;
        }
        fdct8<true>(d, o);
#pragma unroll
        for (int i = 0; i < 8; i++) ws[b][r][i] = o[i];
    }
    __syncthreads();
    // 3. column pass and quantiser; dummy blocks are zeroed
    for (int t = tid; t < nblk * 8; t += 256) {
        const int b = t >> 3, r = t & 7;
        int c, byl, bxl;
        tile_block(g, b, c, byl, bxl);
        const int h = c == 0 ? g.hs : 1, v = c == 0 ? g.vs : 1;
        const int gx = tile * (kTileW / 8) * h / g.hs + bxl, gy = my * v + byl;
        const bool dummy = gx >= g.own_bw[c] || gy >= g.own_bh[c];
        int d[8], o[8];
#pragma unroll
        for (int i = 0; i < 8; i++) d[i] = ws[b][i][r];
        fdct8<false>(d, o);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int k = c * 64 + i * 8 + r;
            const int a = o[i] < 0 ? -o[i] : o[i];
            const int q = (int)__umulhi((unsigned)(a + 4 * (int)g.quant[k]), g.recip[k]);
            ws[b][i][r] = dummy ? 0 : (o[i] < 0 ? -q : q);
        }
    }
    __syncthreads();
    // 4. DC of the dummy blocks: one thread per luma MCU walks its blocks in MCU order
    if (g.hs * g.vs > 1 && tid < kTileW / (8 * g.hs)) {
        int prev = 0;
        for (int v = 0; v < g.vs; v++)
            for (int u = 0; u < g.hs; u++) {
                const int b = v * 16 + tid * g.hs + u;
                const int gx = tile * 16 + tid * g.hs + u, gy = my * g.vs + v;
                if (gx >= g.own_bw[0] || gy >= g.own_bh[0]) ws[b][0][0] = prev;
                else prev = ws[b][0][0];
            }
    }
    __syncthreads();
    // 5. dense rows and mask bytes
    for (int t = tid; t < nblk * 8; t += 256) {
        const int b = t >> 3, r = t & 7;
        int c, byl, bxl;
        tile_block(g, b, c, byl, bxl);
        const int h = c == 0 ? g.hs : 1, v = c == 0 ? g.vs : 1;
        const int gx = tile * (kTileW / 8) * h / g.hs + bxl, gy = my * v + byl;
        unsigned m = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int nat = kNaturalOf[8 * r + i];
            m |= (unsigned)(ws[b][nat >> 3][nat & 7] != 0) << i;
        }
        mbyte[b][r] = (u8)m;
        if (gx < g.bw[c]) {                                            // the last tile of a row may reach past the MCU grid
            const long gb = (long)frame * g.nblocks + g.block_off[c] + (long)gy * g.bw[c] + gx;
            uint4 w;
            w.x = (unsigned)(ws[b][r][0] & 0xffff) | (unsigned)ws[b][r][1] << 16;
            w.y = (unsigned)(ws[b][r][2] & 0xffff) | (unsigned)ws[b][r][3] << 16;
            w.z = (unsigned)(ws[b][r][4] & 0xffff) | (unsigned)ws[b][r][5] << 16;
            w.w = (unsigned)(ws[b][r][6] & 0xffff) | (unsigned)ws[b][r][7] << 16;
            *(uint4 *)(coef + gb * 64 + r * 8) = w;
        }
    }
    if (!masks) return;
    __syncthreads();
    for (int b = tid; b < nblk; b += 256) {
        int c, byl, bxl;
        tile_block(g, b, c, byl, bxl);
        const int h = c == 0 ? g.hs : 1, v = c == 0 ? g.vs : 1;
        const int gx = tile * (kTileW / 8) * h / g.hs + bxl, gy = my * v + byl;
        if (gx >= g.bw[c]) continue;
        const long gb = (long)frame * g.nblocks + g.block_off[c] + (long)gy * g.bw[c] + gx;
        const unsigned long long m = *(const unsigned long long *)&mbyte[b][0];
        masks[gb] = m;
        offsets[gb] = (unsigned)__popcll(m);
    }
}

// popcounts -> exclusive prefix sums, per frame, in place; counts[frame] = the frame's total
__global__ __launch_bounds__(1024) void k_jpeg_scan(unsigned *__restrict__ offsets, long nblocks, unsigned *__restrict__ counts)
{
    __shared__ unsigned wsum[16];
    unsigned *o = offsets + (long)blockIdx.x * nblocks;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned carry = 0;
    for (long base = 0; base < nblocks; base += 4096) {
        const long i0 = base + 4L * threadIdx.x;
        unsigned v[4], s = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) { v[j] = i0 + j < nblocks ? o[i0 + j] : 0; s += v[j]; }
        unsigned inc = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned up = __shfl_up(inc, d, 64);
            if (lane >= d) inc += up;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) { const unsigned x = wsum[w]; before += w < wave ? x : 0; total += x; }
        unsigned ex = carry + before + inc - s;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (i0 + j < nblocks) { o[i0 + j] = ex; ex += v[j]; }
        carry += total;
        __syncthreads();                                               // wsum is rewritten by the next round
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

__global__ __launch_bounds__(256) void k_jpeg_compact(const short *__restrict__ coef, const unsigned long long *__restrict__ masks, const unsigned *__restrict__ offsets,
                                                       long nblocks, long total_blocks, short *__restrict__ values)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x, gb = t >> 3;
    const int r = (int)(t & 7);
    if (gb >= total_blocks) return;
    const unsigned long long m = masks[gb];
    unsigned bits = (unsigned)(m >> (8 * r)) & 0xffu;
    if (!bits) return;
    const long frame = gb / nblocks;
    short *out = values + frame * nblocks * 64 + offsets[gb] + __popcll(m & ((1ull << (8 * r)) - 1));
    const short *blk = coef + gb * 64;
    while (bits) {
        const int i = __ffs(bits) - 1;
        bits &= bits - 1;
        *out++ = blk[kNaturalOf[8 * r + i]];
    }
}

}  // namespace

// coef: n * coef_count dense values, or nullptr (then the sparse outputs are wanted and the dense blocks live in the context's scratch);
// masks, offsets [n * blocks], values [n * coef_count] (frame f's at f * coef_count), counts [n]: all or none
int svk_jpeg_forward(sv_ctx *ctx, const sv_jpeg_enc *plan, const u8 *src, int channels, int n, ptrdiff_t pitch, ptrdiff_t img_stride, int16_t *coef, uint64_t *masks,
                     uint32_t *offsets, int16_t *values, uint32_t *counts, hipStream_t s)
{
    const sv_jpeg_info &info = plan->info;
    JpegEncGeom g = {};
    g.W = info.width; g.H = info.height; g.ncomp = info.components; g.hs = info.h_samp; g.vs = info.v_samp;
    g.mcu_cols = (g.W + 8 * g.hs - 1) / (8 * g.hs);
    const int mcu_rows = (g.H + 8 * g.vs - 1) / (8 * g.vs);
    long off = 0;
    for (int c = 0; c < g.ncomp; c++) {
        const int h = c == 0 ? g.hs : 1, v = c == 0 ? g.vs : 1;
        g.bw[c] = g.mcu_cols * h;
        g.own_bw[c] = (g.W * h + g.hs * 8 - 1) / (g.hs * 8);
        g.own_bh[c] = (g.H * v + g.vs * 8 - 1) / (g.vs * 8);
        g.block_off[c] = off;
        off += (long)g.bw[c] * mcu_rows * v;
    }
    g.nblocks = off;
    for (int i = 0; i < 192; i++) { g.quant[i] = plan->quant[i]; g.recip[i] = plan->recip[i]; }
    if (!coef) {
        const int rc = ctx->jpeg_enc.grow(ctx, (size_t)n * (size_t)off * 64 * sizeof(int16_t));
        if (rc) return rc;
        coef = ctx->jpeg_enc.as<int16_t>();
    }
    const dim3 grid((unsigned)((g.W + kTileW - 1) / kTileW), (unsigned)mcu_rows, (unsigned)n);
    if (channels == 1)
        hipLaunchKernelGGL(k_jpeg_forward<1>, grid, dim3(256), 0, s, src, (long)pitch, (long)img_stride, g, (short *)coef, (unsigned long long *)masks, offsets);
    else
        hipLaunchKernelGGL(k_jpeg_forward<3>, grid, dim3(256), 0, s, src, (long)pitch, (long)img_stride, g, (short *)coef, (unsigned long long *)masks, offsets);
    SV_LAUNCH_CHECK("k_jpeg_forward");
    if (!masks) return SV_OK;
    hipLaunchKernelGGL(k_jpeg_scan, dim3((unsigned)n), dim3(1024), 0, s, offsets, g.nblocks, counts);
    SV_LAUNCH_CHECK("k_jpeg_scan");
    const long total = (long)n * g.nblocks;
    hipLaunchKernelGGL(k_jpeg_compact, dim3((unsigned)((total * 8 + 255) / 256)), dim3(256), 0, s, (const short *)coef, (const unsigned long long *)masks, offsets, g.nblocks,
                       total, (short *)values);
    SV_LAUNCH_CHECK("k_jpeg_compact");
    return SV_OK;
}
