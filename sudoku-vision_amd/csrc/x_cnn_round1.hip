// The round-1 DigitCNN kernels, kept as cross-checks: linked into the test-only libsudokuvision_xcheck.so and never into the product
// (csrc/Makefile).  Independent second implementations of conv2 and fc1 that the tests compare the product's kernels (k3_cnn.hip,
// k3_cnn_h2.hip) with:
//   k_conv_features_wstream : conv2 by Winograd F(2x2, 3x3) on v_mfma_f32_16x16x4_f32   (SV_CNN_X_WINOGRAD)
//   k_conv_features_wsplit  : the same stream on bf16 MFMA, every f32 operand split into three bf16 parts   (SV_CNN_X_WSPLIT)
//   k_fc_head_frame         : fc1 + head with one workgroup per frame   (svx_ctx_set_fc_frame_kernel)
// and their weight images.  The product reaches them through sv_xcheck (sv_internal.h), defined at the end of this file; what the
// kernels share with k3_cnn.hip on the device is in sv_cnn_dev.h.
#include <cstring>

#include "../../include/sudoku_vision_xcheck.h"
#include "sv_cnn_dev.h"
#include "sv_internal.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// k_conv_features_wstream (round 1's default; now a cross-check): conv2 by Winograd F(2x2, 3x3), streamed.  The 7x7 grid of 2x2 output tiles of
// the 14x14 map IS the grid of pooling windows, so per tile:  V = B^T d B over 32 input channels (VALU, 32 add/sub),
// 16 independent GEMMs  M[xi] = V[xi] (tiles x 32) * U[xi] (32 x 64)  on v_mfma_f32_16x16x4_f32, and
// Y = A^T M A + bias, ReLU, 2x2 max -- all four outputs of a tile live in the lane that owns (tile, channel), because
// the 16 GEMMs of one (M tile, N tile) accumulate into 16 register quads of the same lanes.  1568 MFMAs per cell
// instead of 3600; U (G g G^T, 16 x 32 x 16 per wave) stays in 128 VGPRs.  A workgroup owns a contiguous run of cells
// and treats their 49-tile grids as ONE sequence of tiles cut into M tiles of 16 (no 49 -> 64 padding; a per-cell
// variant wasted 23 % of the MFMA rows and needed all of a cell's V, 106 KB, in LDS; here V is two 32-KB slots).
// Winograd reorders the f32 sums: logits differ from the direct kernel by ~1e-6, inside the 1e-4 tolerance
// (tests/test_gpu_parity.py::test_conv_algorithms_agree).
//   step m:  waves 0-3 (one N tile each): 16 GEMMs x 8 k-steps on V[m & 1] for M tile m, output transform, store
//            waves 4-7: B^T d B of M tile m+1 into V[(m+1) & 1] (512 (channel, tile) items = 2 per thread),
//                       conv1 of the next cell whose tiles come up (c1 planes double-buffered by cell parity),
//                       28x28 input of the cell after that (double-buffered too);  one barrier per step.
// The schedule's hazards (a plane is never overwritten while tiles of its previous cell are still to be transformed,
// and so on) are checked exhaustively in tests/test_abi.py::test_winograd_stream_schedule.
// ---------------------------------------------------------------------------------------------------
__host__ __device__ inline long wstream_need(long m, long ncell)   // last cell that M tile m+2 touches
{
    const long c = (16 * (m + 2) + 15) / 49;
    return c < ncell - 1 ? c : ncell - 1;
}

template <bool U8IN>
__global__ __launch_bounds__(512, 2) void k_conv_features_wstream(const void *__restrict__ xin, long B, long cells_per_wg,
                                                                  const float *__restrict__ w1, const float *__restrict__ b1,
                                                                  const float *__restrict__ ureg_img, const float *__restrict__ b2,
                                                                  float *__restrict__ feat)
{
    constexpr int VSLOT = 16 * 32 * 16;       // [xi][ic][tile]
    __shared__ __attribute__((aligned(16))) float lds[2 * IN_CELL + 2 * C1_CELL + 2 * VSLOT];
    float *in_base = lds, *c1_base = lds + 2 * IN_CELL, *v_base = lds + 2 * IN_CELL + 2 * C1_CELL;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool consumer = wave < 4;
    const int nt = wave & 3, ptid = tid & 255;
    const int r16 = lane & 15, q = lane >> 4;

    const long c0 = (long)blockIdx.x * cells_per_wg;
    long ncell = B - c0;
    if (ncell > cells_per_wg) ncell = cells_per_wg;
    if (ncell <= 0) return;
    const int ntiles = (int)ncell * 49, NM = (ntiles + 15) / 16;   // tile arithmetic in 32 bits (a workgroup never owns 2^31 / 49 cells)
    float *featw = feat + c0 * FEAT;                               // this workgroup's first cell

    for (int i = tid; i < 2 * IN_CELL + 2 * C1_CELL + 2 * VSLOT; i += 512) lds[i] = 0.f;
    __syncthreads();

    // Input of a cell -> in_s[c & 1], in two phases so that the global-load latency hides behind the step's other work:
    // stage_load issues one load per value into registers (u8: the cell is 196 dwords, one per thread, 4 pixels of one row
    // each; f32: 784 values, up to 4 per thread), stage_store converts and writes them into the zero-bordered LDS image.
    unsigned sraw[4];
    auto stage_load = [&](long c) {
        if (U8IN) {
            if (ptid < 196) sraw[0] = ((const unsigned *)((const u8 *)xin + (c0 + c) * 784))[ptid];
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (ptid + 256 * j < 784) sraw[j] = __float_as_uint(((const float *)xin)[(c0 + c) * 784 + ptid + 256 * j]);
        }
    };
    auto stage_store = [&](long c) {
        float *in_s = in_base + (c & 1) * IN_CELL;
        if (U8IN) {
            if (ptid < 196) {
                const int y = ptid / 7, x = 4 * (ptid - 7 * y);
                float *d = in_s + (y + 1) * IN_W + x + 1;
#pragma unroll
                for (int j = 0; j < 4; j++) d[j] = glue_norm((u8)(sraw[0] >> (8 * j)));
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int i = ptid + 256 * j;
                if (i < 784) { const int y = i / 28, x = i - y * 28; in_s[(y + 1) * IN_W + x + 1] = __uint_as_float(sraw[j]); }
            }
        }
    };
    auto stage = [&](long c) { stage_load(c); stage_store(c); };
    // conv1 + ReLU + 2x2 max: a producer thread owns one group of 4 output channels (og = ptid / 32, the same for every item
    // and every cell, so its 36 weights + 4 biases stay in registers as {w, w} pairs) and walks the 196 pooled pixels in
    // steps of 32.  The two halves of a wave read the same input patches (LDS broadcast).
    const int og = ptid >> 5, pl = ptid & 31;
    f32x2 wreg[4][9], breg[4];
    auto conv1_load_weights = [&]() {
#pragma unroll
        for (int o = 0; o < 4; o++) {
            const float bias = b1[og * 4 + o];
            breg[o] = (f32x2){bias, bias};
#pragma unroll
            for (int t = 0; t < 9; t++) { const float w = w1[(og * 4 + o) * 9 + t]; wreg[o][t] = (f32x2){w, w}; }
        }
    };
    auto conv1 = [&](long c) {                // producers: in_s[c & 1] -> c1[c & 1]
        const float *in_s = in_base + (c & 1) * IN_CELL;
        float *c1 = c1_base + (c & 1) * C1_CELL + og * 4 * PLANE;
        for (int pp = pl; pp < 196; pp += 32) {
            const int py = pp / 14, px = pp - py * 14;
            // the 4x4 input patch as overlapping horizontal pairs: one v_pk_fma_f32 does the two outputs of a pooling-window row
            f32x2 pr[4][3];
            const float *src = in_s + (2 * py) * IN_W + 2 * px;
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) pr[i][j] = (f32x2){src[i * IN_W + j], src[i * IN_W + j + 1]};
            float *dstp = c1 + (py + 1) * 16 + px + 1;
#pragma unroll
            for (int o = 0; o < 4; o++) {
                f32x2 a0 = breg[o], a1 = breg[o];                    // output rows dy = 0, 1; lanes = dx 0, 1
#pragma unroll
                for (int ky = 0; ky < 3; ky++)
#pragma unroll
                    for (int kx = 0; kx < 3; kx++) {
                        a0 = __builtin_elementwise_fma(wreg[o][ky * 3 + kx], pr[ky][kx], a0);
                        a1 = __builtin_elementwise_fma(wreg[o][ky * 3 + kx], pr[ky + 1][kx], a1);
                    }
                dstp[o * PLANE] = fmaxf(fmaxf(fmaxf(a0[0], a0[1]), fmaxf(a1[0], a1[1])), 0.f);
            }
        }
    };
    auto transform = [&](int m, int first, int last) {   // V[m & 1] = B^T d B for the 16 tiles of M tile m, items [first, last)
        float *Vs = v_base + (m & 1) * VSLOT;
        for (int it = first + ptid; it < last; it += 256) {
            const int ic = it >> 4, tl = it & 15;
            int T = 16 * m + tl;
            if (T > ntiles - 1) T = ntiles - 1;
            const int c = T / 49;
            const int t = T - 49 * c, wy = t / 7, wx = t - 7 * wy;
            const float *d = c1_base + (c & 1) * C1_CELL + ic * PLANE + (2 * wy) * 16 + 2 * wx;
            float tt[4][4];
#pragma unroll
            for (int x = 0; x < 4; x++) {
                const float d0 = d[x], d1 = d[16 + x], d2 = d[32 + x], d3 = d[48 + x];
                tt[0][x] = d0 - d2; tt[1][x] = d1 + d2; tt[2][x] = d2 - d1; tt[3][x] = d1 - d3;
            }
            float *vp = Vs + it;              // (xi*32 + ic)*16 + tl = xi*512 + it
#pragma unroll
            for (int y = 0; y < 4; y++) {
                vp[(y * 4 + 0) * 512] = tt[y][0] - tt[y][2];
                vp[(y * 4 + 1) * 512] = tt[y][1] + tt[y][2];
                vp[(y * 4 + 2) * 512] = tt[y][2] - tt[y][1];
                vp[(y * 4 + 3) * 512] = tt[y][1] - tt[y][3];
            }
        }
    };

    // The two roles run separate loops (one barrier per step in each, so the counts match): register liveness then stays
    // within a role -- U (128 VGPRs) is never live in producer code, nor the conv1 weights in consumer code.
    if (!consumer) {
        conv1_load_weights();
        long conv_done = ncell > 1 ? 1 : 0, staged = conv_done;
        stage(0);
        if (ncell > 1) stage(1);
        __syncthreads();
        conv1(0);
        if (ncell > 1) conv1(1);
        __syncthreads();
        transform(0, 0, 512);
        __syncthreads();
        for (int m = 0; m < NM; m++) {
            const long sc = wstream_need(m + 1, ncell);
            if (sc > staged) stage_load(sc);                      // lands while the transform and conv1 below run
            if (m + 1 < NM) transform(m + 1, 0, 256);
            const long cc = wstream_need(m, ncell);
            if (cc > conv_done) { conv1(cc); conv_done = cc; }
            if (sc > staged) { stage_store(sc); staged = sc; }
            __syncthreads();
        }
        return;
    }

    float ureg[16][8];
#pragma unroll
    for (int xi = 0; xi < 16; xi++)
#pragma unroll
        for (int ks = 0; ks < 8; ks++) ureg[xi][ks] = ureg_img[((nt * 16 + xi) * 8 + ks) * 64 + lane];
    const float bias2 = b2[16 * nt + r16];
    __syncthreads();
    __syncthreads();
    __syncthreads();
    for (int m = 0; m < NM; m++) {
        const float *ap = v_base + (m & 1) * VSLOT + q * 16 + r16;
        f32x4 acc[16];
#pragma unroll
        for (int xi = 0; xi < 16; xi++) acc[xi] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // k-step outermost: consecutive MFMAs hit 16 different accumulators (a dependent 16x16x4 f32 MFMA needs 40
        // cycles, an independent one issues every 32)
#pragma unroll
        for (int ks = 0; ks < 8; ks++)
#pragma unroll
            for (int xi = 0; xi < 16; xi++)
                acc[xi] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[(xi * 32 + 4 * ks) * 16], ureg[xi][ks], acc[xi], 0, 0, 0);
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int T = 16 * m + 4 * q + reg;
            float s0[4], s1[4];
#pragma unroll
            for (int x = 0; x < 4; x++) {
                const float m0 = acc[x][reg], m1 = acc[4 + x][reg], m2 = acc[8 + x][reg], m3 = acc[12 + x][reg];
                s0[x] = m0 + m1 + m2;
                s1[x] = m1 - m2 - m3;
            }
            const float y00 = s0[0] + s0[1] + s0[2], y01 = s0[1] - s0[2] - s0[3];
            const float y10 = s1[0] + s1[1] + s1[2], y11 = s1[1] - s1[2] - s1[3];
            const float pooled = fmaxf(fmaxf(fmaxf(y00, y01), fmaxf(y10, y11)) + bias2, 0.f);
            if (T < ntiles) featw[(unsigned)(T * 64 + 16 * nt + r16)] = pooled;   // (cell c, tile t) sits at c*3136 + t*64 = T*64
        }
        // The MFMA stream above starves the producer waves (f32 MFMA and VALU share the SIMD's issue); what is left of the
        // step is VALU-only, and two waves per SIMD issue VALU faster than one: take half of the next input transform.
        if (m + 1 < NM) transform(m + 1, 256, 512);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------
// k_conv_features_wsplit (experimental, SV_CNN_X_WSPLIT; measured 0.83 ms against the default's 0.81 ms): the Winograd stream
// with its 16 GEMMs on the bf16 matrix pipe at f32 accuracy.
// On gfx950 an f32 MFMA runs at the VALU's rate and blocks the SIMD's VALU issue while it runs (profiles/
// r01_ubench_mfma_valu_coexec.txt); v_mfma_f32_16x16x32_bf16 does 8x the work per cycle and co-issues with VALU work.  Each
// f32 operand is therefore split, without error, into three bf16 parts (x = h + m + l, each the next 8 mantissa bits, by
// truncation: one v_and + one exact v_sub per part), and a product a*b becomes the six partial products
// ah*bh + ah*bm + am*bh + ah*bl + al*bh + am*bm accumulated in f32 -- what is dropped (am*bl, al*bm, al*bl) is below 2^-23 of
// the product, i.e. below f32's own rounding.  U is split once on the host (pack_weights below), V when the input transform
// writes it.  6 MFMAs of K = 32 replace 8 of K = 4: 96 matrix-pipe cycles per (M tile, N tile, xi) instead of 256.
//
// All 8 waves do everything (no producer/consumer split; the 96-register B image of a wave is (N tile nt, half of the xi)):
//   phase A  every thread: one (channel, tile) item of V = B^T d B for M tile m, split and stored as bf16 [part][xi][tile][ic];
//            waves 0-3 first finish M tile m-1: add the other half's partial output transform, bias, ReLU, pool, store
//   barrier
//   phase B  waves 0-3: 48 MFMAs (their 8 xi), partial output transform, then their conv1 share;
//            waves 4-7: conv1 share first, then 48 MFMAs, partial output transform -> LDS
//            (waves w and w+4 share a SIMD, so one's MFMAs run beside the other's VALU work)
//   barrier
// conv1: wave = 4-channel group (weights wave-uniform: scalar registers), lanes = pooled pixels, spread over the 3-4 steps in
// which its plane buffer is free (wsplit_conv1_rounds); input staging in two phases as in k_conv_features_wstream.
// ---------------------------------------------------------------------------------------------------
__host__ __device__ inline int wsplit_conv1_rounds(long m, long tc, int done, int total)
{
    if (16 * m + 15 < 49 * (tc - 2) + 48) return 0;          // M tile m (transformed in this step's phase A) still short of cell tc-2's last tile
    const long left = (49 * tc) / 16 - m;                      // steps m .. F-1, F = first M tile that touches cell tc
    const int remaining = total - done;
    return left <= 1 ? remaining : (int)((remaining + left - 1) / left);
}

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

template <bool U8IN>
__global__ __launch_bounds__(512, 2) void k_conv_features_wsplit(const void *__restrict__ xin, long B, long cells_per_wg,
                                                                 const float *__restrict__ w1, const float *__restrict__ b1,
                                                                 const uint4 *__restrict__ usplit, const float *__restrict__ b2,
                                                                 float *__restrict__ feat)
{
    constexpr int VROW = 80;                  // bytes per (xi, tile): 32 bf16 channels + 16 B of bank skew
    constexpr int VPLANE = 16 * VROW;         // one xi: 16 tiles
    constexpr int VPART = 16 * VPLANE;        // one bf16 part: 16 xi
    __shared__ __attribute__((aligned(16))) float lds[2 * IN_CELL + 2 * C1_CELL];
    __shared__ __attribute__((aligned(16))) unsigned char v3[3 * VPART];
    __shared__ float ypart[4][16][64];        // partial output transforms of waves 4-7: [N tile][4 tiles x 4 values][lane]
    __shared__ __attribute__((aligned(16))) float w1s[32][12];   // conv1 weights [0..8] and bias [9] (broadcast ds_reads; wave-uniform rows)
    float *in_base = lds, *c1_base = lds + 2 * IN_CELL;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nt = wave & 3, xh = wave >> 2;
    const int r16 = lane & 15, q = lane >> 4;

    const long c0 = (long)blockIdx.x * cells_per_wg;
    long ncell = B - c0;
    if (ncell > cells_per_wg) ncell = cells_per_wg;
    if (ncell <= 0) return;
    const int ntiles = (int)ncell * 49, NM = (ntiles + 15) / 16;
    float *featw = feat + c0 * FEAT;

    uint4 breg[8][3];                         // [xi within this wave's half][part]: B[k = 8q + j][col r16] of U[xi], oc = 16nt + r16
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
        for (int p = 0; p < 3; p++) breg[j][p] = usplit[((nt * 16 + 8 * xh + j) * 3 + p) * 64 + lane];
    const float bias2 = b2[16 * nt + r16];
    for (int i = tid; i < 2 * IN_CELL + 2 * C1_CELL; i += 512) lds[i] = 0.f;
    for (int i = tid; i < 3 * VPART / 4; i += 512) ((unsigned *)v3)[i] = 0;
    for (int i = tid; i < 320; i += 512) {
        const int oc = i / 10, t = i - 10 * oc;
        const float w = t < 9 ? w1[oc * 9 + t] : b1[oc];
        w1s[oc][t] = w;
    }
    __syncthreads();

    unsigned sraw[2];
    auto stage_load = [&](long c) {
        if (U8IN) {
            if (tid < 196) sraw[0] = ((const unsigned *)((const u8 *)xin + (c0 + c) * 784))[tid];
        } else {
#pragma unroll
            for (int j = 0; j < 2; j++)
                if (tid + 512 * j < 784) sraw[j] = __float_as_uint(((const float *)xin)[(c0 + c) * 784 + tid + 512 * j]);
        }
    };
    auto stage_store = [&](long c) {
        float *in_s = in_base + (c & 1) * IN_CELL;
        if (U8IN) {
            if (tid < 196) {
                const int y = tid / 7, x = 4 * (tid - 7 * y);
                float *d = in_s + (y + 1) * IN_W + x + 1;
#pragma unroll
                for (int j = 0; j < 4; j++) d[j] = glue_norm((u8)(sraw[0] >> (8 * j)));
            }
        } else {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int i = tid + 512 * j;
                if (i < 784) { const int y = i / 28, x = i - y * 28; in_s[(y + 1) * IN_W + x + 1] = __uint_as_float(sraw[j]); }
            }
        }
    };
    constexpr int C1_ROUNDS = 4;              // 196 pooled pixels in rounds of 64 lanes; the wave is the 4-channel group
    auto conv1 = [&](long c, int r0, int r1) {
        const float *in_s = in_base + (c & 1) * IN_CELL;
        float *c1 = c1_base + (c & 1) * C1_CELL + wave * 4 * PLANE;
        for (int pp = lane + 64 * r0; pp < 196 && pp < 64 * r1; pp += 64) {
            const int py = pp / 14, px = pp - py * 14;
            // plain v_fma_f32 here, not v_pk_fma_f32: a packed f32 op issued beside the other wave's MFMAs costs ~20 cycles more
            float pt[4][4];
            const float *src = in_s + (2 * py) * IN_W + 2 * px;
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) pt[i][j] = src[i * IN_W + j];
            float *dstp = c1 + (py + 1) * 16 + px + 1;
#pragma unroll
            for (int o = 0; o < 4; o++) {
                const float *w = w1s[wave * 4 + o];
                float a00 = w[9], a01 = w[9], a10 = w[9], a11 = w[9];
#pragma unroll
                for (int ky = 0; ky < 3; ky++)
#pragma unroll
                    for (int kx = 0; kx < 3; kx++) {
                        const float wv = w[ky * 3 + kx];
                        a00 = __builtin_fmaf(wv, pt[ky][kx], a00);
                        a01 = __builtin_fmaf(wv, pt[ky][kx + 1], a01);
                        a10 = __builtin_fmaf(wv, pt[ky + 1][kx], a10);
                        a11 = __builtin_fmaf(wv, pt[ky + 1][kx + 1], a11);
                    }
                dstp[o * PLANE] = fmaxf(fmaxf(fmaxf(a00, a01), fmaxf(a10, a11)), 0.f);
            }
        }
    };
    // one (channel, tile) item of V = B^T d B for M tile m, each value split into three bf16 parts
    auto transform = [&](int m) {
        const int ic = tid >> 4, tl = tid & 15;
        int T = 16 * m + tl;
        if (T > ntiles - 1) T = ntiles - 1;
        const int c = T / 49;
        const int t = T - 49 * c, wy = t / 7, wx = t - 7 * wy;
        const float *d = c1_base + (c & 1) * C1_CELL + ic * PLANE + (2 * wy) * 16 + 2 * wx;
        float tt[4][4];
#pragma unroll
        for (int x = 0; x < 4; x++) {
            const float d0 = d[x], d1 = d[16 + x], d2 = d[32 + x], d3 = d[48 + x];
            tt[0][x] = d0 - d2; tt[1][x] = d1 + d2; tt[2][x] = d2 - d1; tt[3][x] = d1 - d3;
        }
        unsigned char *vp = v3 + tl * VROW + ic * 2;
#pragma unroll
        for (int y = 0; y < 4; y++) {
            const float v4[4] = {tt[y][0] - tt[y][2], tt[y][1] + tt[y][2], tt[y][2] - tt[y][1], tt[y][1] - tt[y][3]};
#pragma unroll
            for (int x = 0; x < 4; x++) {
                const float v = v4[x];
                const unsigned uh = __float_as_uint(v) & 0xffff0000u;
                const float r = v - __uint_as_float(uh);                       // exact
                const unsigned um = __float_as_uint(r) & 0xffff0000u;
                const float r2 = r - __uint_as_float(um);                      // exact; its top 16 bits are the third part
                unsigned char *o = vp + (y * 4 + x) * VPLANE;
                *(unsigned short *)o = (unsigned short)(uh >> 16);
                *(unsigned short *)(o + VPART) = (unsigned short)(um >> 16);
                *(unsigned short *)(o + 2 * VPART) = (unsigned short)(__float_as_uint(r2) >> 16);
            }
        }
    };

    // prologue: cells 0 and 1 convolved, cell 2 staged
    long conv_done = ncell > 1 ? 1 : 0;
    int conv_round = 0;
    stage_load(0); stage_store(0);
    __syncthreads();
    conv1(0, 0, C1_ROUNDS);
    if (ncell > 1) { stage_load(1); stage_store(1); }
    __syncthreads();
    if (ncell > 1) conv1(1, 0, C1_ROUNDS);
    if (ncell > 2) { stage_load(2); stage_store(2); }
    __syncthreads();

    float p0[4][4];                           // waves 0-3: this wave's partial output transform, [tile reg][y00, y01, y10, y11]
    auto finish = [&](int m) {                // waves 0-3: M tile m's outputs = own partial + the other half's (in LDS)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int T = 16 * m + 4 * q + reg;
            const float y00 = p0[reg][0] + ypart[nt][reg * 4 + 0][lane], y01 = p0[reg][1] + ypart[nt][reg * 4 + 1][lane];
            const float y10 = p0[reg][2] + ypart[nt][reg * 4 + 2][lane], y11 = p0[reg][3] + ypart[nt][reg * 4 + 3][lane];
            const float pooled = fmaxf(fmaxf(fmaxf(y00, y01), fmaxf(y10, y11)) + bias2, 0.f);
            if (T < ntiles) featw[(unsigned)(T * 64 + 16 * nt + r16)] = pooled;
        }
    };

    for (int m = 0; m < NM; m++) {
        // ---- phase A
        if (xh == 0 && m > 0) finish(m - 1);
        transform(m);
        __syncthreads();
        // ---- phase B
        const long tc = conv_done + 1;
        const int rounds = tc < ncell ? wsplit_conv1_rounds(m, tc, conv_round, C1_ROUNDS) : 0;
        const bool completes = rounds > 0 && conv_round + rounds == C1_ROUNDS;
        if (completes && tc + 1 < ncell) stage_load(tc + 1);
        if (xh == 1 && rounds > 0) conv1(tc, conv_round, conv_round + rounds);

        f32x4 acc[8];
        {
            const unsigned char *ap = v3 + r16 * VROW + q * 16;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const unsigned char *a = ap + (8 * xh + j) * VPLANE;
                const bf16x8_t ah = __builtin_bit_cast(bf16x8_t, *(const uint4 *)a);
                const bf16x8_t am = __builtin_bit_cast(bf16x8_t, *(const uint4 *)(a + VPART));
                const bf16x8_t al = __builtin_bit_cast(bf16x8_t, *(const uint4 *)(a + 2 * VPART));
                const bf16x8_t bh = __builtin_bit_cast(bf16x8_t, breg[j][0]), bm = __builtin_bit_cast(bf16x8_t, breg[j][1]),
                               bl = __builtin_bit_cast(bf16x8_t, breg[j][2]);
                f32x4 s = {0.f, 0.f, 0.f, 0.f};                               // smallest terms first
                s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bm, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bh, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bm, s, 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, s, 0, 0, 0);
            }
        }
        // partial output transform over this wave's two rows of the 4x4 xi grid (xi = 4x + y, x in {2xh, 2xh+1}):
        // r[x][0] = M[x][0] + M[x][1] + M[x][2], r[x][1] = M[x][1] - M[x][2] - M[x][3];
        // Y[0][b] = r[0][b] + r[1][b] + r[2][b], Y[1][b] = r[1][b] - r[2][b] - r[3][b]
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const float ra0 = acc[0][reg] + acc[1][reg] + acc[2][reg], ra1 = acc[1][reg] - acc[2][reg] - acc[3][reg];   // first row of the half
            const float rb0 = acc[4][reg] + acc[5][reg] + acc[6][reg], rb1 = acc[5][reg] - acc[6][reg] - acc[7][reg];   // second row
            if (xh == 0) {                    // rows x = 0, 1: Y[0][b] += r0 + r1, Y[1][b] += r1
                p0[reg][0] = ra0 + rb0; p0[reg][1] = ra1 + rb1; p0[reg][2] = rb0; p0[reg][3] = rb1;
            } else {                          // rows x = 2, 3: Y[0][b] += r2, Y[1][b] += -r2 - r3
                ypart[nt][reg * 4 + 0][lane] = ra0; ypart[nt][reg * 4 + 1][lane] = ra1;
                ypart[nt][reg * 4 + 2][lane] = -ra0 - rb0; ypart[nt][reg * 4 + 3][lane] = -ra1 - rb1;
            }
        }
        if (xh == 0 && rounds > 0) conv1(tc, conv_round, conv_round + rounds);
        if (rounds > 0) {
            conv_round += rounds;
            if (completes) {
                if (tc + 1 < ncell) stage_store(tc + 1);
                conv_done = tc;
                conv_round = 0;
            }
        }
        __syncthreads();
    }
    if (xh == 0) finish(NM - 1);
}

// ---------------------------------------------------------------------------------------------------
// k_fc_head_frame: one 512-thread workgroup per 81 cells (one frame), i.e. one per CU at 256 frames, so the MFMA work is
// spread evenly, and the fc1 weight image is fetched ONCE per workgroup: each 32-wide K stage (16 KB) goes global ->
// registers -> LDS (double-buffered, one barrier per stage) and all waves read their B operands from LDS.  The plain
// k_fc_head streams the whole 1.6 MB image through every wave and is bound by L1 bandwidth (and by 324 workgroups on 256 CUs).
// 81 cells = 6 M tiles: waves 0-3 take M tiles 0-3 (all 8 N tiles), waves 4-7 take M tiles 4,5 split in two halves of N,
// which gives every SIMD (waves s and s+4) three half-tile jobs.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void k_fc_head_frame(const float *__restrict__ feat, long B, const float *__restrict__ w1reg,
                                                       const float *__restrict__ b1, const float *__restrict__ w2,
                                                       const float *__restrict__ b2, float *__restrict__ logits,
                                                       u8 *__restrict__ digits, float *__restrict__ conf, const int *__restrict__ run_if_set)
{
    if (run_if_set && *run_if_set == 0) return;                       // (as k_fc_head: under SV_CNN_AUTO the f16-pair kernels took this batch)
    constexpr int CELLS = 81, ROWS = 96, CH = 4, WPT = CH * 8 * 64 / 512;   // WPT float4 of weights per thread per stage                      // cells per workgroup, padded rows, 16-wide chunks per stage
    __shared__ __attribute__((aligned(16))) f32x4 wt[2][CH * 8 * 64]; // 2 x 32 KB weight stages
    __shared__ float hs[ROWS][129];
    __shared__ float w2s[10][128];
    __shared__ float lg[ROWS][12];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int mt = wave < 4 ? wave : 4 + ((wave - 4) >> 1);           // M tile of this wave
    const int t0 = wave < 4 ? 0 : 4 * ((wave - 4) & 1);               // first N tile
    const int nt_cnt = wave < 4 ? 8 : 4;                              // N tiles of this wave
    const long cellbase = (long)blockIdx.x * CELLS;
    long crow = cellbase + mt * 16 + r;
    const long last = (cellbase + CELLS < B ? cellbase + CELLS : B) - 1;
    if (crow > last) crow = last;
    const f32x4 *ap = (const f32x4 *)(feat + crow * FEAT + 4 * q);
    const f32x4 *wp = (const f32x4 *)w1reg;                           // [196][8][64] float4

    sv_fc2_stage<512>(w2s, w2, tid);

    f32x4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; t++) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

    constexpr int NSTAGE = 196 / CH;                                  // 49 stages of 2048 float4 = 4 per thread
    f32x4 wreg[WPT], areg[CH];
#pragma unroll
    for (int j = 0; j < WPT; j++) wreg[j] = wp[512 * j + tid];
#pragma unroll
    for (int c = 0; c < CH; c++) areg[c] = ap[c * 4];
#pragma unroll
    for (int j = 0; j < WPT; j++) wt[0][512 * j + tid] = wreg[j];
    __syncthreads();

    for (int st = 0; st < NSTAGE; st++) {
        const int cur = st & 1;
        f32x4 a[CH];
#pragma unroll
        for (int c = 0; c < CH; c++) a[c] = areg[c];
        if (st + 1 < NSTAGE) {                                        // next stage: global -> registers while this one computes
#pragma unroll
            for (int j = 0; j < WPT; j++) wreg[j] = wp[(long)(st + 1) * (CH * 8 * 64) + 512 * j + tid];
#pragma unroll
            for (int c = 0; c < CH; c++) areg[c] = ap[((st + 1) * CH + c) * 4];
        }
#pragma unroll
        for (int c = 0; c < CH; c++) {
            if (nt_cnt == 8) {
                f32x4 b[8];
#pragma unroll
                for (int t = 0; t < 8; t++) b[t] = wt[cur][(c * 8 + t) * 64 + lane];
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int t = 0; t < 8; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c][e], b[t][e], acc[t], 0, 0, 0);
            } else {
                f32x4 b[4];
#pragma unroll
                for (int t = 0; t < 4; t++) b[t] = wt[cur][(c * 8 + t0 + t) * 64 + lane];
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c][e], b[t][e], acc[t], 0, 0, 0);
            }
        }
        if (st + 1 < NSTAGE) {
#pragma unroll
            for (int j = 0; j < WPT; j++) wt[cur ^ 1][512 * j + tid] = wreg[j];
        }
        __syncthreads();
    }

    // acc[t][reg]: cell row mt*16 + 4q + reg, hidden unit 16*(t0 + t) + r
#pragma unroll
    for (int t = 0; t < 8; t++)
        if (t < nt_cnt) {
            const int n = 16 * (t0 + t) + r;
            const float bias = b1[n];
#pragma unroll
            for (int reg = 0; reg < 4; reg++) hs[mt * 16 + 4 * q + reg][n] = fmaxf(acc[t][reg] + bias, 0.f);
        }
    __syncthreads();
    for (int it = tid; it < CELLS * 10; it += 512) {                  // fc2
        const int cl = it / 10, j = it - 10 * cl;
        const float sacc = sv_fc2_logit(hs[cl], w2s, b2, j);
        lg[cl][j] = sacc;
        if (cellbase + cl < B) logits[(cellbase + cl) * 10 + j] = sacc;
    }
    __syncthreads();
    if (tid < CELLS && cellbase + tid < B) sv_digit_conf(lg[tid], cellbase + tid, digits, conf);
}

// The Winograd weight images of conv2.weight c2w [64][32][3][3], on top of what svk_pack_weights_f32mfma uploads
int pack_weights(sv_weights &w, const float *c2w)
{
    int rc;
    // Winograd F(2x2,3x3) weights U = G g G^T (computed in double), as [nt][xi][ks][lane]: oc = 16nt + (lane&15), ic = 4ks + (lane>>4)
    std::vector<float> wino((size_t)4 * 16 * 8 * 64);
    // the same U split without error into three bf16 parts (each the next 8 mantissa bits, by truncation) for
    // k_conv_features_wsplit: [nt][xi][part][lane][j], oc = 16nt + (lane&15), ic = 8*(lane>>4) + j
    std::vector<uint16_t> wsplit((size_t)4 * 16 * 3 * 64 * 8);
    const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    for (int oc = 0; oc < 64; oc++)
        for (int ic = 0; ic < 32; ic++) {
            const float *g = c2w + (oc * 32 + ic) * 9;
            double Gg[4][3], U[4][4];
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 3; j++) Gg[i][j] = G[i][0] * g[j] + G[i][1] * g[3 + j] + G[i][2] * g[6 + j];
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 4; j++) U[i][j] = Gg[i][0] * G[j][0] + Gg[i][1] * G[j][1] + Gg[i][2] * G[j][2];
            const int nt = oc >> 4, lane = (oc & 15) + 16 * (ic & 3), ks = ic >> 2;
            for (int xi = 0; xi < 16; xi++) {
                const float u = (float)U[xi >> 2][xi & 3];
                wino[(((size_t)nt * 16 + xi) * 8 + ks) * 64 + lane] = u;
                float rest = u;
                for (int part = 0; part < 3; part++) {
                    uint32_t bits;
                    memcpy(&bits, &rest, 4);
                    bits &= 0xffff0000u;
                    float piece;
                    memcpy(&piece, &bits, 4);
                    rest -= piece;                                        // exact
                    wsplit[((((size_t)nt * 16 + xi) * 3 + part) * 64 + (oc & 15) + 16 * (ic >> 3)) * 8 + (ic & 7)] = (uint16_t)(bits >> 16);
                }
            }
        }
    if ((rc = sv_upload(w, &w.conv2_wino, wino.data(), wino.size()))) return rc;
    if ((rc = sv_upload(w, &w.conv2_wsplit, wsplit.data(), wsplit.size()))) return rc;
    return SV_OK;
}

// the selections sv_ctx_set_cnn_kernels takes on top of the product's, and the kernel family each names
bool select_conv(int which, sv_cnn_algo *algo)
{
    if (which == SV_CNN_X_WINOGRAD) *algo = SV_ALGO_X_WINOGRAD;
    else if (which == SV_CNN_X_WSPLIT) *algo = SV_ALGO_X_WSPLIT;
    else return false;
    return true;
}

// SV_ALGO_X_WINOGRAD / SV_ALGO_X_WSPLIT: a contiguous run of cells per workgroup, one workgroup per CU; x -> ctx->features
void launch_conv(sv_ctx *ctx, sv_cnn_algo conv_algo, const void *x, bool x_is_u8, long B, hipStream_t s)
{
    const sv_weights &w = ctx->w;
    long cpw = (B + ctx->num_cus - 1) / ctx->num_cus;
    if (cpw < 1) cpw = 1;
    const int grid_s = (int)((B + cpw - 1) / cpw);
    if (conv_algo == SV_ALGO_X_WSPLIT) {
        if (x_is_u8)
            hipLaunchKernelGGL(k_conv_features_wsplit<true>, dim3(grid_s), dim3(512), 0, s, x, B, cpw, w.conv1_w, w.conv1_b, (const uint4 *)w.conv2_wsplit, w.conv2_b, ctx->features.as<float>());
        else
            hipLaunchKernelGGL(k_conv_features_wsplit<false>, dim3(grid_s), dim3(512), 0, s, x, B, cpw, w.conv1_w, w.conv1_b, (const uint4 *)w.conv2_wsplit, w.conv2_b, ctx->features.as<float>());
    } else {
        if (x_is_u8)
            hipLaunchKernelGGL(k_conv_features_wstream<true>, dim3(grid_s), dim3(512), 0, s, x, B, cpw, w.conv1_w, w.conv1_b, w.conv2_wino, w.conv2_b, ctx->features.as<float>());
        else
            hipLaunchKernelGGL(k_conv_features_wstream<false>, dim3(grid_s), dim3(512), 0, s, x, B, cpw, w.conv1_w, w.conv1_b, w.conv2_wino, w.conv2_b, ctx->features.as<float>());
    }
}

void launch_fc_frame(sv_ctx *ctx, long B, float *logits, u8 *digits, float *conf, const int *run_if_set, hipStream_t s)
{
    const sv_weights &w = ctx->w;
    hipLaunchKernelGGL(k_fc_head_frame, dim3((unsigned)((B + 80) / 81)), dim3(512), 0, s, ctx->features.as<float>(), B, w.fc1_wreg, w.fc1_b, w.fc2_w, w.fc2_b, logits, digits, conf, run_if_set);
}

sv_xcheck_ops ops = {select_conv, pack_weights, launch_conv, launch_fc_frame};   // (not const: a const table would be emitted for the device as well)

}  // namespace

const sv_xcheck_ops *const sv_xcheck = &ops;

extern "C" int svx_ctx_set_fc_frame_kernel(sv_ctx *ctx, int on)
{
    if (!ctx) return sv_fail(SV_ERR_BAD_ARG, "svx_ctx_set_fc_frame_kernel: NULL context");
    ctx->x_fc_frame = on != 0;
    return SV_OK;
}
