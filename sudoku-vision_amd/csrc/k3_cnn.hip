// K3 -- DigitCNN.forward (ml/model.py:34-42, eval mode) on MI355X: the f32-MFMA kernels and the small stages around the CNN.
// (The default conv/fc pair -- f32-grade arithmetic on the f16 matrix pipe -- is k3_cnn_h2.hip, the bf16 configuration k3_cnn_bf16.hip;
// svk_cnn_forward at the end of this file picks the family, see sv_ctx_set_precision and sv_ctx_set_cnn_kernels.)
//
//   k_conv_features_pc : true f32 throughout, the reference's own numeric range: what runs when the loaded weights or an f32 input
//        leave the range the f16-pair kernels carry exactly (and for misaligned 8-bit buffers).  Persistent, one 512-thread workgroup per
//        CU working through PAIRS of cells.  conv1 (1->32, 3x3, pad 1) + ReLU + 2x2 max-pool on the VALU into zero-bordered 16x16
//        planes in LDS; conv2 (32->64) as an implicit GEMM on v_mfma_f32_16x16x4_f32:
//        M = 4 pooling windows x 4 positions, N = 16 output channels, K = 4 input channels of one
//        3x3 tap per instruction.  A comes straight from the LDS planes (one ds_read_b32 with an
//        immediate offset per step, no im2col buffer); B (all 288x32 weights a wave needs) stays in
//        144 VGPRs for the life of the kernel.  The 16x16 accumulator holds the 4 positions of a
//        pooling window in the 4 registers of one lane, so bias + ReLU + max-pool are 3 v_max and
//        never leave the lane.  Output: features [cell][window 49][oc 64] f32.
//   k_fc_head : fc1 (3136->128) on the same MFMA with cells as M (16 cells per wave, weights streamed per wave); bias + ReLU, fc2 (128->10),
//        argmax (pipeline/run.py:142) and softmax[argmax] (run.py:141-143) are sv_fc_tail, the tail of every fc head (sv_fc_head.h).
//   k_softmax_topk, k_preprocess_cells: the run_v2 top-k epilogue and run.py's preprocess_cell (scope rows N3, N1).
//   (The round-1 kernels the tests compare these with -- k_conv_features_wstream / _wsplit, k_fc_head_frame -- are x_cnn_round1.hip, in the
//        test-only libsudokuvision_xcheck.so alone; svk_cnn_forward reaches them through sv_xcheck, sv_internal.h.)
//
// Weight images are packed on the host by svk_pack_weights_f32mfma (below) into exactly the
// per-lane register order the kernels load.
#include "sv_fc_head.h"
#include "sv_internal.h"
#include "sv_n1_preprocess.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// k_conv_features_pc: one 512-thread workgroup per CU, software-pipelined over cell pairs with ONE
// barrier per pair (producer/consumer wave specialisation).
//   waves 0-3 (consumers): conv2 of pair i on the MFMA pipe, from c1[i & 1]           (weights in VGPRs)
//   waves 4-7 (producers): conv1 of pair i+1 on the VALU into c1[(i+1) & 1], and the 28x28 inputs of
//                          pair i+2 into in_s[i & 1]
// The matrix pipe and the vector pipe of a SIMD run side by side, so the consumers never leave the
// MFMA stream for conv1 or for input staging.  LDS: 2 x 65,792 (conv1 planes) + 2 x 7,200 (inputs) B.
// ---------------------------------------------------------------------------------------------------
struct GaussTaps { float k[11]; };

template <bool U8IN>
__global__ __launch_bounds__(512, 2) void k_conv_features_pc(const void *__restrict__ xin, long B,
                                                             const float *__restrict__ w1, const float *__restrict__ b1,
                                                             const float *__restrict__ w2reg, const float *__restrict__ b2,
                                                             float *__restrict__ feat, const int *__restrict__ run_if_set)
{
    if (run_if_set && *run_if_set == 0) return;      // (svk_cnn_forward: the f16-pair kernels took this batch)
    __shared__ __attribute__((aligned(16))) float lds[4 * IN_CELL + 4 * C1_CELL];
    float *in_base = lds;                 // [2 buffers][2 cells][900]
    float *c1_base = lds + 4 * IN_CELL;   // [2 buffers][2 cells][32][257]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool consumer = wave < 4;
    const int np = (wave >> 1) & 1, par = wave & 1;   // consumer roles
    const int pw = wave & 3, ptid = tid & 255;        // producer roles

    float breg[2][72];
    float bias2_0 = 0.f, bias2_1 = 0.f;
    if (consumer) {
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int ks = 0; ks < 72; ks++) breg[t][ks] = w2reg[((np * 2 + t) * 72 + ks) * 64 + lane];
        bias2_0 = b2[32 * np + (lane & 15)];
        bias2_1 = b2[32 * np + 16 + (lane & 15)];
    }
    for (int i = tid; i < 4 * IN_CELL + 4 * C1_CELL; i += 512) lds[i] = 0.f;   // zero borders, for good
    __syncthreads();

    const long npairs = (B + 1) / 2;
    const long first = blockIdx.x, stride = gridDim.x;
    const long iters = first < npairs ? (npairs - first + stride - 1) / stride : 0;

    auto stage = [&](long it) {          // producers: inputs of local iteration `it` -> in_s[it & 1]
        const long pair = first + it * stride;
        float *in_s = in_base + (it & 1) * 2 * IN_CELL;
        for (int i = ptid; i < 2 * 784; i += 256) {
            const int cl = i / 784, p = i - cl * 784, y = p / 28, x = p - y * 28;
            long cg = pair * 2 + cl;
            if (cg >= B) cg = B - 1;
            float v;
            if (U8IN) v = glue_norm(((const u8 *)xin)[cg * 784 + p]);
            else v = ((const float *)xin)[cg * 784 + p];
            in_s[cl * IN_CELL + (y + 1) * IN_W + x + 1] = v;
        }
    };
    auto conv1 = [&](long it) {          // producers: in_s[it & 1] -> c1[it & 1]
        const float *in_s = in_base + (it & 1) * 2 * IN_CELL;
        float *c1 = c1_base + (it & 1) * 2 * C1_CELL;
        for (int rnd = 0; rnd < 7; rnd++) {
            const int idx = rnd * 64 + lane;
            if (idx < 392) {
                const int cl = idx / 196, pp = idx - cl * 196, py = pp / 14, px = pp - py * 14;
                float patch[4][4];
                const float *src = in_s + cl * IN_CELL + (2 * py) * IN_W + 2 * px;
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) patch[i][j] = src[i * IN_W + j];
                float *dstp = c1 + cl * C1_CELL + (py + 1) * 16 + px + 1;
#pragma unroll
                for (int o = 0; o < 8; o++) {
                    const int oc = pw * 8 + o;
                    const float *w = w1 + oc * 9;
                    const float bias = b1[oc];
                    float m = -3.0e38f;
#pragma unroll
                    for (int dy = 0; dy < 2; dy++)
#pragma unroll
                        for (int dx = 0; dx < 2; dx++) {
                            float acc = bias;
#pragma unroll
                            for (int ky = 0; ky < 3; ky++)
#pragma unroll
                                for (int kx = 0; kx < 3; kx++) acc = __builtin_fmaf(w[ky * 3 + kx], patch[dy + ky][dx + kx], acc);
                            m = fmaxf(m, acc);
                        }
                    dstp[oc * PLANE] = fmaxf(m, 0.f);
                }
            }
        }
    };

    // prologue: fill the pipeline
    if (!consumer && iters > 0) stage(0);
    __syncthreads();
    if (!consumer) {
        if (iters > 0) conv1(0);
        if (iters > 1) stage(1);
    }
    __syncthreads();

    for (long it = 0; it < iters; it++) {
        if (consumer) {
            const long pair = first + it * stride;
            const float *c1 = c1_base + (it & 1) * 2 * C1_CELL;
            for (int j = par; j < 25; j += 2) {
                const int i16 = lane & 15, q = lane >> 4;
                int g = 4 * j + (i16 >> 2);
                if (g > 97) g = 97;
                const int cl = g >= 49 ? 1 : 0, wl = g - 49 * cl, wy = wl / 7, wx = wl - 7 * wy, s = i16 & 3;
                const float *ap = c1 + cl * C1_CELL + q * 8 * PLANE + (2 * wy + (s >> 1)) * 16 + 2 * wx + (s & 1);
                f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 72; ks++) {
                    const int tap = ks >> 3, icb = ks & 7;
                    const float a = ap[icb * PLANE + (tap / 3) * 16 + (tap % 3)];
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, breg[0][ks], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, breg[1][ks], acc1, 0, 0, 0);
                }
                const int gw = 4 * j + q;
                if (gw < 98) {
                    const int ocl = gw >= 49 ? 1 : 0, owl = gw - 49 * ocl;
                    const long cg = pair * 2 + ocl;
                    if (cg < B) {
                        float *o = feat + cg * FEAT + owl * 64 + 32 * np + i16;
                        o[0] = fmaxf(fmaxf(fmaxf(acc0[0], acc0[1]), fmaxf(acc0[2], acc0[3])) + bias2_0, 0.f);
                        o[16] = fmaxf(fmaxf(fmaxf(acc1[0], acc1[1]), fmaxf(acc1[2], acc1[3])) + bias2_1, 0.f);
                    }
                }
            }
        } else {
            if (it + 1 < iters) conv1(it + 1);
            if (it + 2 < iters) stage(it + 2);
        }
        __syncthreads();
    }
}

// 64 cells per workgroup, 16 per wave; K = 3136 in 196 chunks of 16.
__global__ __launch_bounds__(256) void k_fc_head(const float *__restrict__ feat, long B, const float *__restrict__ w1reg,
                                                 const float *__restrict__ b1, const float *__restrict__ w2,
                                                 const float *__restrict__ b2, float *__restrict__ logits,
                                                 u8 *__restrict__ digits, float *__restrict__ conf, const int *__restrict__ run_if_set)
{
    if (run_if_set && *run_if_set == 0) return;
    __shared__ float hs[4][16][129];
    __shared__ float w2s[10][128];
    __shared__ float lg[4][16][12];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const sv_fc_lane l = sv_fc_wave_tile(lane, wave, B);
    const f32x4 *ap = (const f32x4 *)(feat + l.crow * FEAT + 4 * l.q);
    const f32x4 *bp = (const f32x4 *)w1reg + lane;

    sv_fc2_stage<256>(w2s, w2, tid);

    f32x4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; t++) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // explicit two-deep register pipeline: the 9 loads of chunk c+2 are issued before the MFMAs of chunk c
    f32x4 a0 = ap[0], a1 = ap[4], wb0[8], wb1[8];
#pragma unroll
    for (int t = 0; t < 8; t++) { wb0[t] = bp[t * 64]; wb1[t] = bp[(8 + t) * 64]; }
    for (int c = 0; c < 196; c += 2) {
        f32x4 na0 = a0, na1 = a1, nwb0[8], nwb1[8];
        const int c2 = c + 2 < 196 ? c + 2 : c, c3 = c + 3 < 196 ? c + 3 : c + 1;   // (tail: harmless re-loads)
        na0 = ap[c2 * 4];
#pragma unroll
        for (int t = 0; t < 8; t++) nwb0[t] = bp[(c2 * 8 + t) * 64];
#pragma unroll
        for (int e = 0; e < 4; e++)
#pragma unroll
            for (int t = 0; t < 8; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], wb0[t][e], acc[t], 0, 0, 0);
        na1 = ap[c3 * 4];
#pragma unroll
        for (int t = 0; t < 8; t++) nwb1[t] = bp[(c3 * 8 + t) * 64];
#pragma unroll
        for (int e = 0; e < 4; e++)
#pragma unroll
            for (int t = 0; t < 8; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], wb1[t][e], acc[t], 0, 0, 0);
        a0 = na0; a1 = na1;
#pragma unroll
        for (int t = 0; t < 8; t++) { wb0[t] = nwb0[t]; wb1[t] = nwb1[t]; }
    }

    sv_fc_tail<8>(hs[wave], 0, [=](int t, int reg) { return acc[t][reg]; }, b1, w2s, b2, lg[wave], l.cell0, B, true, logits, digits, conf);
}

// preprocess_cell (pipeline/run.py:73-95) as a stand-alone call: one wave per cell, u8 in -> u8 {0,255} out
__global__ __launch_bounds__(256) void k_preprocess_cells(const u8 *__restrict__ cells, long B, GaussTaps taps, u8 *__restrict__ out)
{
    __shared__ N1Scratch sc[4];
    __shared__ float tile[4][IN_CELL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long c = (long)blockIdx.x * 4 + wave;
    if (c >= B) return;
    n1_preprocess_cell(cells + c * 784, tile[wave], sc[wave], lane, taps.k);
    wave_lds_fence();
    for (int i = lane; i < 784; i += 64) {
        const int y = i / 28, x = i - 28 * y;
        out[c * 784 + i] = tile[wave][(y + 1) * IN_W + x + 1] < 0.f ? 255 : 0;
    }
}

}  // namespace

int svk_pack_weights_f32mfma(sv_weights &w, const float *c2w, const float *f1w)
{
    // conv2: [np][t][ks][lane]; lane -> oc = 32np + 16t + (lane&15), ic = icb + 8*(lane>>4); ks = tap*8 + icb
    std::vector<float> w2(2 * 2 * 72 * 64);
    for (int np = 0; np < 2; np++)
        for (int t = 0; t < 2; t++)
            for (int ks = 0; ks < 72; ks++)
                for (int lane = 0; lane < 64; lane++) {
                    const int oc = 32 * np + 16 * t + (lane & 15), tap = ks >> 3, ic = (ks & 7) + 8 * (lane >> 4);
                    w2[((np * 2 + t) * 72 + ks) * 64 + lane] = c2w[(oc * 32 + ic) * 9 + tap];
                }
    // fc1: [chunk][t][lane][e]; feature index k' = 16*chunk + 4*(lane>>4) + e = window*64 + oc;
    // the reference flattens NCHW: k = oc*49 + window (ml/model.py:38)
    std::vector<float> f1((size_t)196 * 8 * 64 * 4);
    for (int c = 0; c < 196; c++)
        for (int t = 0; t < 8; t++)
            for (int lane = 0; lane < 64; lane++)
                for (int e = 0; e < 4; e++) {
                    const int kp = 16 * c + 4 * (lane >> 4) + e, win = kp >> 6, oc = kp & 63, n = 16 * t + (lane & 15);
                    f1[(((size_t)c * 8 + t) * 64 + lane) * 4 + e] = f1w[(size_t)n * 3136 + oc * 49 + win];
                }
    int rc;
    if ((rc = sv_upload(w, &w.conv2_wreg, w2.data(), w2.size()))) return rc;
    if ((rc = sv_upload(w, &w.fc1_wreg, f1.data(), f1.size()))) return rc;
    return sv_xcheck ? sv_xcheck->pack_weights(w, c2w) : SV_OK;
}

int svk_preprocess_cells(const u8 *cells, long B, u8 *out, hipStream_t s)
{
    GaussTaps taps;
    sv_gaussian_taps_f32(11, taps.k);
    hipLaunchKernelGGL(k_preprocess_cells, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, cells, B, taps, out);
    SV_LAUNCH_CHECK("k_preprocess_cells");
    return SV_OK;
}

// F.softmax + topk (pipeline/run_v2.py:165-178): one thread per cell, 10 logits in registers, k selection passes.  A pass starts from
// the lowest untaken class and moves only to a strictly greater one: equal probabilities come lowest class first, and a row whose
// probabilities do not compare (a NaN or +inf logit, all -inf: den is NaN and so is every prob written) still gets k distinct classes.
__global__ __launch_bounds__(256) void k_softmax_topk(const float *__restrict__ logits, long B, int k, u8 *__restrict__ index, float *__restrict__ prob)
{
    const long cell = (long)blockIdx.x * 256 + threadIdx.x;
    if (cell >= B) return;
    float p[10];
    float best = -INFINITY;
#pragma unroll
    for (int j = 0; j < 10; j++) { p[j] = logits[cell * 10 + j]; best = fmaxf(best, p[j]); }
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < 10; j++) { p[j] = expf(p[j] - best); den += p[j]; }
    unsigned taken = 0;
    for (int r = 0; r < k; r++) {
        float top = -1.f;
        int arg = -1;
#pragma unroll
        for (int j = 0; j < 10; j++)
            if (!(taken >> j & 1) && (arg < 0 || p[j] > top)) { top = p[j]; arg = j; }
        taken |= 1u << arg;
        index[cell * k + r] = (u8)arg;
        prob[cell * k + r] = top / den;
    }
}

int svk_softmax_topk(const float *logits, long B, int k, u8 *index, float *prob, hipStream_t s)
{
    hipLaunchKernelGGL(k_softmax_topk, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, logits, B, k, index, prob);
    SV_LAUNCH_CHECK("k_softmax_topk");
    return SV_OK;
}

// Which conv/fc kernels run (sv_ctx_set_cnn_kernels; include/sudoku_vision_hip.h):
//   SV_CNN_AUTO (default)  the f16 hi/lo operand-pair kernels (k3_cnn_h2.hip) whenever the loaded weights keep every activation inside their
//                          range, else the f32-MFMA kernels below, which have the reference's own range (svk_pack_weights_h2 decides; f32
//                          inputs are range-checked on the device per call)
//   SV_CNN_F16PAIR / SV_CNN_F32MFMA   one of the two, unconditionally
//   (where sv_xcheck is set, i.e. in libsudokuvision_xcheck.so only) SV_CNN_X_WINOGRAD, SV_CNN_X_WSPLIT: the round-1 Winograd stream on
//   f32 / on split-bf16 MFMA, and svx_ctx_set_fc_frame_kernel for the one-workgroup-per-frame fc kernel (x_cnn_round1.hip)
static sv_cnn_algo effective_algo(const sv_ctx *ctx)
{
    sv_cnn_algo x;
    if (ctx->cnn_kernels == SV_CNN_F16PAIR) return SV_ALGO_F16PAIR;
    if (ctx->cnn_kernels == SV_CNN_F32MFMA) return SV_ALGO_F32MFMA;
    if (sv_xcheck && sv_xcheck->select_conv(ctx->cnn_kernels, &x)) return x;
    return ctx->w.h2_in_range ? SV_ALGO_F16PAIR : SV_ALGO_F32MFMA;
}

extern "C" int sv_ctx_set_cnn_kernels(sv_ctx *ctx, int which)
{
    if (!ctx) return sv_fail(SV_ERR_BAD_ARG, "sv_ctx_set_cnn_kernels: NULL context");
    bool ok = which == SV_CNN_AUTO || which == SV_CNN_F16PAIR || which == SV_CNN_F32MFMA;
    sv_cnn_algo x;
    ok = ok || (sv_xcheck && sv_xcheck->select_conv(which, &x));
    if (!ok) return sv_fail(SV_ERR_BAD_ARG, "sv_ctx_set_cnn_kernels: unknown selection %d", which);
    ctx->cnn_kernels = which;
    return SV_OK;
}

extern "C" int sv_conv_kernel_info(sv_ctx *ctx, int *algo, int *mfma_f32_conv2_per_cell, int *mfma_f32_conv1_per_cell, int *mfma_f16_conv_per_cell,
                                   int *mfma_f16_fc_per_cell)
{
    if (!ctx || !algo || !mfma_f32_conv2_per_cell || !mfma_f32_conv1_per_cell || !mfma_f16_conv_per_cell || !mfma_f16_fc_per_cell)
        return sv_fail(SV_ERR_BAD_ARG, "sv_conv_kernel_info: NULL argument");
    const sv_cnn_algo a = effective_algo(ctx);
    *algo = a;
    // f32 Winograd: 49 tiles x 16 xi x 8 k-steps x 4 N tiles / 16 tiles per M tile; f32 direct: 196 positions / 16 x 72 k-steps x 4 N tiles
    *mfma_f32_conv2_per_cell = a == SV_ALGO_X_WINOGRAD ? 1568 : (a == SV_ALGO_F32MFMA ? 3600 : 0);
    *mfma_f32_conv1_per_cell = 0;
    // f16 pairs: conv2 13 M tiles x 9 taps x 4 N tiles x 3 products + conv1 13 M tiles x 8 N tiles x 2; fc1 98 k-steps x 8 N tiles x 3 per 16 cells
    *mfma_f16_conv_per_cell = a == SV_ALGO_F16PAIR ? 13 * 9 * 4 * 3 + 13 * 8 * 2 : 0;
    *mfma_f16_fc_per_cell = a == SV_ALGO_F16PAIR ? 98 * 8 * 3 / 16 : 0;
    return SV_OK;
}

// |x| of an f32 input batch against the range the f16-pair kernels carry exactly: flag = 0 (use them) when lo <= max|x| <= hi and no
// value is NaN/Inf, else 1 (the f32-MFMA kernels).  One pass over the input; both kernel pairs are launched and the one the flag does
// not name returns at once, so the decision never costs a host synchronisation.
__global__ __launch_bounds__(256) void k_input_range(const float *__restrict__ x, long n, float lo, float hi, int *__restrict__ flag)
{
    __shared__ float part[4];
    float m = 0.f;
    bool bad = false;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float v = fabsf(x[i]);
        bad |= !(v <= hi);                                          // also NaN
        m = fmaxf(m, v);
    }
    for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
        if (m >= lo) atomicOr(flag + 1, 1);                         // some block saw a value of at least lo
    }
}
__global__ void k_input_range_finish(int *flag)                     // flag[0] |= nothing reached lo (all-tiny input); flag[1] is scratch
{
    if (flag[1] == 0) flag[0] = 1;
}

// The whole CNN forward of a batch: run.py's preprocess_cell pass when asked for, then the bf16 configuration or the SV_PREC_F32 family
// effective_algo names.
int svk_cnn_forward(sv_ctx *ctx, const void *x, bool x_is_u8, int glue, long B, float *logits, u8 *digits, float *conf, hipStream_t s)
{
    const sv_weights &w = ctx->w;
    const long npairs = (B + 1) / 2;
    if (ctx->precision == SV_PREC_BF16 && !x_is_u8)
        return sv_fail(SV_ERR_UNSUPPORTED, "sv_cnn_forward_f32: the bf16 configuration takes 8-bit cells (sv_cnn_forward_cells_u8 / sv_frames_to_digits)");
    if (x_is_u8 && glue == SV_GLUE_RUNPY) {      // run.py's preprocess_cell as its own pass; its {0,255} output then takes the plain glue
        int rc = svk_preprocess_cells((const u8 *)x, B, ctx->cells2.as<u8>(), s);
        if (rc) return rc;
        x = ctx->cells2.p;
    }
    if (ctx->precision == SV_PREC_BF16) return svk_cnn_forward_bf16(ctx, (const u8 *)x, B, logits, digits, conf, s);
    sv_cnn_algo conv_algo = effective_algo(ctx);
    // (the kernels that read 8-bit cells as dwords need a 4-byte-aligned buffer; a misaligned one takes the direct f32 kernel)
    if (x_is_u8 && ((uintptr_t)x & 3)) conv_algo = SV_ALGO_F32MFMA;
    const int *flag = nullptr;                   // device flag: 0 = the f16-pair kernels run, 1 = the f32-MFMA kernels (both are launched)
    if (conv_algo == SV_ALGO_F16PAIR && !x_is_u8 && ctx->cnn_kernels == SV_CNN_AUTO) {
        // 8-bit cells are in [-1, 1] after the glue (what svk_pack_weights_h2 sized the activations for); f32 input can be anything
        const int rc = ctx->range_flag.grow(ctx, 2 * sizeof(int));       // (sv_ctx_reserve has done it where a capture follows)
        if (rc) return rc;
        int *range_flag = ctx->range_flag.as<int>();
        SV_HIP(hipMemsetAsync(range_flag, 0, 2 * sizeof(int), s));
        const long n = B * 784;
        hipLaunchKernelGGL(k_input_range, dim3((unsigned)(n / 4096 + 1 < 1024 ? n / 4096 + 1 : 1024)), dim3(256), 0, s, (const float *)x, n, w.h2_x_lo, w.h2_x_hi, range_flag);
        hipLaunchKernelGGL(k_input_range_finish, dim3(1), dim3(1), 0, s, range_flag);
        SV_LAUNCH_CHECK("k_input_range");
        flag = range_flag;
    }
    if (conv_algo == SV_ALGO_F16PAIR) {
        const int rc = svk_cnn_forward_h2(ctx, x, x_is_u8, B, logits, digits, conf, flag, s);
        if (rc || !flag) return rc;
    }
    if (sv_xcheck && (conv_algo == SV_ALGO_X_WSPLIT || conv_algo == SV_ALGO_X_WINOGRAD)) {
        sv_time_scope ts(ctx, SVK_CONV_FEATURES, s);
        sv_xcheck->launch_conv(ctx, conv_algo, x, x_is_u8, B, s);
    } else {
        const int grid_pc = (int)(npairs < (long)ctx->num_cus ? npairs : (long)ctx->num_cus);
        sv_time_scope ts(ctx, SVK_CONV_FEATURES, s);
        if (x_is_u8)
            hipLaunchKernelGGL(k_conv_features_pc<true>, dim3(grid_pc), dim3(512), 0, s, x, B, w.conv1_w, w.conv1_b, w.conv2_wreg, w.conv2_b, ctx->features.as<float>(), flag);
        else
            hipLaunchKernelGGL(k_conv_features_pc<false>, dim3(grid_pc), dim3(512), 0, s, x, B, w.conv1_w, w.conv1_b, w.conv2_wreg, w.conv2_b, ctx->features.as<float>(), flag);
    }
    SV_LAUNCH_CHECK("k_conv_features");
    sv_time_scope ts(ctx, SVK_FC_HEAD, s);
    if (sv_xcheck && ctx->x_fc_frame && B >= 81 * 64)       // (svx_ctx_set_fc_frame_kernel) enough frames to give most CUs a workgroup
        sv_xcheck->launch_fc_frame(ctx, B, logits, digits, conf, flag, s);
    else
        hipLaunchKernelGGL(k_fc_head, dim3((unsigned)((B + 63) / 64)), dim3(256), 0, s, ctx->features.as<float>(), B, w.fc1_wreg, w.fc1_b, w.fc2_w, w.fc2_b, logits, digits, conf, flag);
    SV_LAUNCH_CHECK("k_fc_head");
    return SV_OK;
}
