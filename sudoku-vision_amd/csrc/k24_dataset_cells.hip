// K24 -- a data set of PNG cells -> model input (ml/datasets.py:18-46 preprocess_cell, :69-92 and :141-164 the two __getitem__; ml/evaluate.py:67 the
// plain gray read): the filtered bytes of n small PNG files, each of its own geometry, -> n cells of 28 x 28 as u8 and as float(u8) / 255.  The host
// half (host_png.cpp) parses and inflates; this is everything after that, and the cell never goes back to HBM in between.
//
//   k_dataset_cells<LARGE>   64 threads: ONE WAVE PER CELL, the whole cell in LDS.
//     1. the record is checked (svds::refuse, sv_dataset_rec.h: the rules sv_dataset_check_records reports on the host).  A refused record
//        writes zeros and SV_CELLS_STATUS_REFUSED and reads nothing else.
//     2. the filtered rows are copied into LDS, row r at raw + r * PITCH.
//     3. unfilter: K19's skewed wavefront with lane = row.  A cell has at most 64 rows, so it is one stripe, and at most 512 bytes a row, so it
//        is one chunk: in step s lane l does byte s - l of its row, takes `above` from lane l - 1's last result by one cross-lane move (lane 0:
//        zero, nothing is above the image) and keeps its own last 8 bytes and the 8 above them in two 64-bit registers, so `left` and
//        `above-left` are shifts.  row_bytes + H - 1 steps whatever the rows' filters are; a filter byte above 4 is None (svpng::unfilter_byte).
//     4. svpng::expand_gray of every pixel -> the gray plane (or straight into the 28 x 28 cell when the file is 28 x 28).
//     5. cv2.resize(img, (28, 28)): the two axis tables (28 entries each, sv_resize_axis) by 56 lanes, then sv_resize_px per pixel.
//     6. SV_CELLS_DATASET: n1_preprocess_cell (sv_n1_preprocess.h, the body of k_preprocess_cells) in the LDS the raw rows no longer need;
//        its THRESH_BINARY result inverted is the data set's 255 - x.
//     7. out_u8, out_f32 = float(u8) / 255.0f (__fdiv_rn: a division, as torch's), status.
//   PITCH is the only thing the two instances differ in: 69 for cells of row_bytes <= 64 (28 x 28 gray: 28; every gray cell of 8 bits), 517 for
//   the rest (up to 64 px of RGBA16).  The records are on the device, so the host cannot size the LDS from the launch's largest row_bytes
//   without reading them back; instead both instances are launched with a workgroup per cell, and a workgroup whose cell is of the other class
//   leaves after reading its 16-byte record.  A batch of 28 x 28 gray cells is charged 16.6 KB a wave, not 38.6 KB (9 against 4 waves a CU).
//   43 VGPRs, no scratch.  The body is NOT in a loop over cells: in one, the compiler hoists N1's per-lane indices out of it and wants 430 registers.
//   PITCH % 8 == 5, so (PITCH - 1) / 4 is odd and the skewed wave's 64 byte addresses fall into distinct banks, as K19's kPitch.
//
// Robustness: every index below is bounded by the checked geometry (W, H <= 64, row_bytes <= 512 < PITCH when LARGE, <= 64 < PITCH else), the
// stream's extent by filtered_size, the palette index by n_palettes, the palette's entry count by 256; loops run over the checked geometry alone;
// a wave never waits for another (one wave a workgroup, no __syncthreads, no atomics, no global scratch).  status is written by the cell's own
// wave, so nothing has to zero it first (and a graph replay writes it anew: the hipMemsetAsync trap of k_png_clear's comment does not arise).
#include "sv_dataset_rec.h"
#include "sv_internal.h"
#include "sv_n1_preprocess.h"
#include "sv_png_pixel.h"

namespace {

struct CellTaps { float k[11]; };

template <int PITCH>
struct CellLds {
    union {
        u8 raw[SV_CELLS_MAX_SIDE * PITCH];                           // the filtered, then unfiltered rows: dead once the gray plane is written
        struct { N1Scratch sc; float tile[IN_CELL]; } n1;           // step 6
    };
    u8 plane[SV_CELLS_MAX_SIDE * SV_CELLS_MAX_SIDE];                 // gray, W dense
    u8 cell[784];
    int axis[2][28][3];                                             // x then y: offset and the two weights
};

template <bool LARGE>
__global__ __launch_bounds__(64) void k_dataset_cells(const u8 *__restrict__ filtered, size_t filtered_size, const sv_dataset_record *__restrict__ records, long n,
                                                      const u8 *__restrict__ palettes, int n_palettes, int mode, CellTaps taps, u8 *__restrict__ out_u8,
                                                      float *__restrict__ out_f32, uint32_t *__restrict__ status)
{
    constexpr int PITCH = LARGE ? SV_CELLS_MAX_ROW_BYTES + 5 : 64 + 5;
    static_assert(PITCH % 8 == 5, "the skewed wave's bank spread");
    __shared__ CellLds<PITCH> L;
    const int lane = threadIdx.x;
    const long c = blockIdx.x;                                       // grid = n
    const sv_dataset_record rec = records[c];
    svds::Geom g;
    const bool refused = svds::refuse(rec, filtered_size, n_palettes, g) != nullptr;
    if (LARGE && (refused || g.row_bytes <= 64)) return;       // the small instance's
    if (!LARGE && !refused && g.row_bytes > 64) return;
    if (refused) {
        for (int i = lane; i < 784; i += 64) {
            if (out_u8) out_u8[c * 784 + i] = 0;
            if (out_f32) out_f32[c * 784 + i] = 0.f;
        }
        if (lane == 0) status[c] = SV_CELLS_STATUS_REFUSED;
        return;
    }
    const u8 *src = filtered + g.offset;
    const int stride = 1 + g.row_bytes, rb = g.row_bytes, H = g.H, W = g.W;
    for (int i = lane; i < H * stride; i += 64) {
        const int r = i / stride, x = i - r * stride;
        if (x) L.raw[r * PITCH + x - 1] = src[i];
    }
    const bool active = lane < H;
    const unsigned f = active ? src[lane * stride] : 0u;         // unfilter_byte takes a value above 4 as None
    wave_lds_fence();
    {
        uint64_t mine = 0, above = 0;                            // the last 8 bytes of this row and of the row above it, newest lowest
        const int back = 8 * (g.bpp - 1);
        u8 *own = L.raw + lane * PITCH;
        for (int s = 0; s < rb + H - 1; s++) {
            const int x = s - lane;
            const unsigned handed = __shfl_up((unsigned)(mine & 255u), 1);
            if (active && x >= 0 && x < rb) {
                const unsigned b = lane == 0 ? 0u : handed;
                const unsigned v = svpng::unfilter_byte(f, own[x], (unsigned)(mine >> back) & 255u, b, (unsigned)(above >> back) & 255u);
                mine = mine << 8 | v;
                above = above << 8 | b;
                own[x] = (u8)v;
            }
        }
    }
    wave_lds_fence();
    const bool direct = W == 28 && H == 28;
    bool bad = false;
    {
        const bool paletted = g.color_type == 3;
        const u8 *pal = paletted ? palettes + (size_t)rec.palette * SV_PNG_PALETTE_STRIDE : nullptr;     // refuse(): palette < n_palettes
        const unsigned pal_n = paletted ? min(256u, *(const uint32_t *)(pal + 768)) : 0u;
        const svpng::Expand e = {g.color_type, g.bit_depth, g.channels};
        u8 *dst = direct ? L.cell : L.plane;
        for (int i = lane; i < H * W; i += 64) {
            const int y = i / W, x = i - y * W;
            const unsigned px = svpng::expand_gray(e, L.raw + y * PITCH, x, pal, pal_n);
            bad |= (px >> 8) != 0;
            dst[i] = (u8)px;
        }
    }
    if (!direct) {
        if (lane < 56) {
            const int a = lane >= 28, d = lane - 28 * a;
            int o, w0, w1;
            sv_resize_axis(a ? H : W, 28, d, o, w0, w1);
            L.axis[a][d][0] = o; L.axis[a][d][1] = w0; L.axis[a][d][2] = w1;
        }
        wave_lds_fence();
        for (int i = lane; i < 784; i += 64) {
            const int y = i / 28, x = i - 28 * y;
            const u8 *plane = L.plane;
            L.cell[i] = (u8)sv_resize_px(L.axis[0][x][0], L.axis[0][x][1], L.axis[0][x][2], L.axis[1][y][0], L.axis[1][y][1], L.axis[1][y][2], H, W,
                                         [=](int tx, int ty) { return (int)plane[ty * W + tx]; });
        }
    }
    wave_lds_fence();
    if (mode == SV_CELLS_DATASET) {
        // inlined: as a call it would charge this kernel the callee ABI's whole register file
        [[clang::always_inline]] n1_preprocess_cell(L.cell, L.n1.tile, L.n1.sc, lane, taps.k);
        wave_lds_fence();
    }
    for (int i = lane; i < 784; i += 64) {
        const int y = i / 28, x = i - 28 * y;
        // n1's tile holds -1 where THRESH_BINARY gave 255: the data set's 255 - x is 0 there
        const int v = mode == SV_CELLS_DATASET ? (L.n1.tile[(y + 1) * IN_W + x + 1] < 0.f ? 0 : 255) : (int)L.cell[i];
        if (out_u8) out_u8[c * 784 + i] = (u8)v;
        if (out_f32) out_f32[c * 784 + i] = __fdiv_rn((float)v, 255.0f);
    }
    const bool any_bad = __any(bad);
    if (lane == 0) status[c] = any_bad ? SV_CELLS_STATUS_PALETTE : 0u;
}

}  // namespace

int svk_dataset_cells(sv_ctx *ctx, const u8 *filtered, size_t filtered_size, const sv_dataset_record *records, long n, const u8 *palettes, int n_palettes, int mode,
                      u8 *out_u8, float *out_f32, uint32_t *status, hipStream_t s)
{
    CellTaps taps;
    sv_gaussian_taps_f32(11, taps.k);
    hipLaunchKernelGGL(k_dataset_cells<false>, dim3((unsigned)n), dim3(64), 0, s, filtered, filtered_size, records, n, palettes, n_palettes, mode, taps, out_u8, out_f32,
                       status);
    SV_LAUNCH_CHECK("k_dataset_cells<small>");
    (void)ctx;
    hipLaunchKernelGGL(k_dataset_cells<true>, dim3((unsigned)n), dim3(64), 0, s, filtered, filtered_size, records, n, palettes, n_palettes, mode, taps, out_u8, out_f32, status);
    SV_LAUNCH_CHECK("k_dataset_cells<large>");
    return SV_OK;
}
