// K12 -- DigitCNNv3Light.forward (ml/model_v3.py:232-282) and EmptyClassifier.forward (:285-320), eval mode, on MI355X, true f32 throughout.
//
// One launch per forward.  One 256-thread workgroup carries one cell from its input to its logits; every activation stays in LDS
// (the largest, 24 x 14 x 14, is 26 KB with its zero border), weights are read from L2 as MFMA B-operand images.  All matrix work is
// v_mfma_f32_16x16x4_f32; the conv core (LDS planes, K loop, weight image) is sv_conv_f32.h's, the scheme of k8_cnn_v3.hip.
//
//   conv_in : the first convolution of either model (1 input channel, 28x28).  With one channel the K of the implicit GEMM is the tap:
//        K = 4 taps per instruction, 3 instructions per tile (taps 9..11 carry zero weights).  The shared scheme (K = 4 input channels of
//        one tap) would spend 9 instructions on three zero planes.
//   conv_lds : the other convolutions, on the shared K loop, LDS to LDS.
//   Max pooling is an epilogue: in a pooled layer the 16 rows of an M tile are four 2x2 windows, row 4 w + r = pixel r of window w.  The
//        MFMA result then has the four pixels of one window in the four accumulator registers of one lane, and the pool is three fmaxf
//        in registers.  relu(max(x) + b) = max(relu(x + b)): + b and relu are monotone and round monotonically, so the bias and ReLU are
//        applied once, after the max.  Input planes of pooled layers are padded to 8 mod 32 floats (sv_conv_plane), the others to 16.
//   N = 24 (Light's first layer) is two 16-channel tiles whose last 8 columns have zero weights and are not stored.
//   Light: conv_in(24) -> pool -> conv_lds(24 -> 48) -> pool -> conv_lds(48 -> 96) -> mean over the 49 positions in order 0..48 ->
//        sv_head_tail (features and fc.weight zero-padded from 96 to sv_fc2_logit's 128: fmaf(0, 0, s) = s).
//   Empty: conv_in(16) -> pool -> conv_lds(16 -> 32) -> pool -> flatten [c][y][x] -> Linear(1568 -> 32): thread (j = tid & 31, s = tid >> 5)
//        sums segment s (196 terms, in order) of output j with fmaf, eight segments are added in order 0..7, + bias, ReLU ->
//        Linear(32 -> 1) by one thread.
// A cell is computed by the same instructions in the same order whatever shares its batch: results are batch-independent bit for bit.
#include <cmath>
#include <vector>

#include "sv_conv_f32.h"
#include "sv_internal.h"

namespace {

constexpr int IN_PLANE = sv_conv_plane(28, 16);   // 912: 30 x 30 zero-bordered input
constexpr int P14 = sv_conv_plane(14, 8);         // 264: 16 x 16 zero-bordered plane, read by a pooled layer
constexpr int P7 = sv_conv_plane(7, 16);          // 112: 9 x 9 zero-bordered plane, read by an unpooled layer

// First layer: sin (30 x 30) -> conv3x3 to 16 NT channels + bias + ReLU + maxpool 2x2 -> sout [COUT][P14] (16 x 16 zero-bordered planes).
// wp: [NT][3 kk][64 lane]: lane l holds w'[oc = 16 nt + (l & 15)][tap = 4 kk + (l >> 4)], zero where tap > 8 or oc >= COUT.  bias [16 NT].
template <int NT, int COUT>
__device__ __forceinline__ void conv_in(const float *sin, const float *__restrict__ wp, const float *__restrict__ bias, float *sout, int wave, int lane)
{
    const int m = lane & 15, kq = lane >> 4;
    int off[3];
#pragma unroll
    for (int kk = 0; kk < 3; kk++) {
        const int tap = 4 * kk + kq < 9 ? 4 * kk + kq : 8;      // taps 9..11: zero weight, any address inside the plane
        off[kk] = (tap / 3) * 30 + tap % 3;
    }
    for (int nt = 0; nt < NT; nt++) {
        float b[3];
#pragma unroll
        for (int kk = 0; kk < 3; kk++) b[kk] = wp[(nt * 3 + kk) * 64 + lane];
        const int oc = nt * 16 + m;
        const float bv = bias[oc];
        for (int t = wave; t < 49; t += 4) {                    // 196 windows = 49 tiles of 4
            const int qa = 4 * t + (m >> 2), r = m & 3;
            const int base = (2 * (qa / 14) + (r >> 1)) * 30 + 2 * (qa % 14) + (r & 1);
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < 3; kk++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(sin[base + off[kk]], b[kk], acc, 0, 0, 0);
            // D: column lane & 15 = oc, rows 4 (lane >> 4) + r = pixel r of window 4 t + (lane >> 4)
            const int q = 4 * t + kq;
            const float v = fmaxf(fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3])) + bv, 0.f);
            if (oc < COUT) sout[oc * P14 + (q / 14 + 1) * 16 + q % 14 + 1] = v;
        }
    }
}

// sin [CIN][IPLANE] zero-bordered (HIN+2)^2 planes -> conv3x3 to 16 NT channels + bias + ReLU (+ maxpool 2x2 when POOL) -> sout: channel oc at
// oc * OPLANE, output pixel (y, x) at (y + OB) * OPW + x + OB.  wp: sv_pack_conv_image's [NT][CIN/4][9][64 lane].  MB M-tiles share each B value.
template <int CIN, int NT, int HIN, int IPLANE, int MB, bool POOL, int OPLANE, int OPW, int OB>
__device__ __forceinline__ void conv_lds(const float *sin, const float *__restrict__ wp, const float *__restrict__ bias, float *sout, int wave, int lane)
{
    constexpr int PW = HIN + 2, HO = POOL ? HIN / 2 : HIN, NOUT = HO * HO, TILES = POOL ? (NOUT + 3) / 4 : (NOUT + 15) / 16;
    constexpr int GROUPS = (TILES + MB - 1) / MB, G4 = CIN / 4;
    static_assert(CIN % 4 == 0, "tiling");
    const int m = lane & 15, kq = lane >> 4;
    for (int item = wave; item < GROUPS * NT; item += 4) {
        const int grp = item % GROUPS, nt = item / GROUPS;
        int base[MB];
#pragma unroll
        for (int i = 0; i < MB; i++) {
            const int tile = grp * MB + i;                      // tiles and rows past the plane recompute its last output; they are not stored
            if (POOL) {
                int q = tile * 4 + (m >> 2);
                q = q < NOUT ? q : NOUT - 1;
                base[i] = kq * IPLANE + (2 * (q / HO) + ((m & 3) >> 1)) * PW + 2 * (q % HO) + (m & 1);
            } else {
                int p = tile * 16 + m;
                p = p < NOUT ? p : NOUT - 1;
                base[i] = kq * IPLANE + (p / HO) * PW + p % HO;
            }
        }
        f32x4 acc[MB];
#pragma unroll
        for (int i = 0; i < MB; i++) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        sv_conv_kloop<G4, 3, PW, IPLANE, MB>(sin, base, wp + nt * (G4 * 9 * 64) + lane, acc);
        const int oc = nt * 16 + m;
        const float bv = bias[oc];
        float *o = sout + oc * OPLANE + OB * OPW + OB;
#pragma unroll
        for (int i = 0; i < MB; i++) {
            const int tile = grp * MB + i;
            if (POOL) {
                const int q = tile * 4 + kq;
                const float v = fmaxf(fmaxf(fmaxf(acc[i][0], acc[i][1]), fmaxf(acc[i][2], acc[i][3])) + bv, 0.f);
                if (q < NOUT) o[(q / HO) * OPW + q % HO] = v;
            } else {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int p = tile * 16 + kq * 4 + r;
                    if (p < NOUT) o[(p / HO) * OPW + p % HO] = fmaxf(acc[i][r] + bv, 0.f);
                }
            }
        }
    }
}

// x: B cells -> logits [B][10], features [B][96] (or NULL), digits / conf (or NULL)
template <bool U8IN>
__global__ __launch_bounds__(256) void k_light(const void *__restrict__ x, const float *__restrict__ w1, const float *__restrict__ b1, const float *__restrict__ w2,
                                               const float *__restrict__ b2, const float *__restrict__ w3, const float *__restrict__ b3,
                                               const float *__restrict__ fcw, const float *__restrict__ fcb, float temperature, float *__restrict__ features,
                                               float *__restrict__ logits, u8 *__restrict__ digits, float *__restrict__ conf)
{
    constexpr int A1 = 24 * P14, A2 = 48 * P7, A3 = 96 * 49;
    static_assert(A3 <= A1, "conv3's output takes conv1's place");
    __shared__ float sm[IN_PLANE + A1 + A2];
    __shared__ float f[128];
    float *sin = sm, *act1 = sm + IN_PLANE, *act2 = act1 + A1, *act3 = act1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long cell = blockIdx.x;

    for (int i = tid; i < IN_PLANE + A1 + A2; i += 256) sm[i] = 0.f;
    if (tid < 128) f[tid] = 0.f;
    __syncthreads();
    sv_conv_load_input<U8IN, 1, 28, IN_PLANE>(x, cell, sin, tid);
    __syncthreads();
    conv_in<2, 24>(sin, w1, b1, act1, wave, lane);
    __syncthreads();
    conv_lds<24, 3, 14, P14, 4, true, P7, 9, 1>(act1, w2, b2, act2, wave, lane);
    __syncthreads();
    conv_lds<48, 6, 7, P7, 2, false, 49, 7, 0>(act2, w3, b3, act3, wave, lane);
    __syncthreads();
    if (tid < 96) {
        const float *p = act3 + tid * 49;
        float s = 0.f;
        for (int i = 0; i < 49; i++) s += p[i];
        s = s / 49.f;
        f[tid] = s;
        if (features) features[cell * 96 + tid] = s;
    }
    sv_head_tail(f, fcw, fcb, temperature, cell, logits, digits, conf);
}

// x: B cells -> logit [B].  f1w: [8 s][49 i4][32 j][4 e] = classifier.1.weight[j][196 s + 4 i4 + e]
template <bool U8IN>
__global__ __launch_bounds__(256) void k_empty(const void *__restrict__ x, const float *__restrict__ w1, const float *__restrict__ b1, const float *__restrict__ w2,
                                               const float *__restrict__ b2, const float *__restrict__ f1w, const float *__restrict__ f1b,
                                               const float *__restrict__ f2w, const float *__restrict__ f2b, float *__restrict__ logit)
{
    constexpr int A1 = 16 * P14, A2 = 1568;
    __shared__ __attribute__((aligned(16))) float sm[IN_PLANE + A1 + A2];
    __shared__ float part[256], hid[32];
    float *sin = sm, *act1 = sm + IN_PLANE, *act2 = act1 + A1;
    static_assert((IN_PLANE + A1) % 4 == 0, "act2 is read as float4");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long cell = blockIdx.x;

    for (int i = tid; i < IN_PLANE + A1; i += 256) sm[i] = 0.f;
    __syncthreads();
    sv_conv_load_input<U8IN, 1, 28, IN_PLANE>(x, cell, sin, tid);
    __syncthreads();
    conv_in<1, 16>(sin, w1, b1, act1, wave, lane);
    __syncthreads();
    conv_lds<16, 2, 14, P14, 4, true, 49, 7, 0>(act1, w2, b2, act2, wave, lane);
    __syncthreads();
    {
        const int j = tid & 31, s = tid >> 5;
        const f32x4 *wv = (const f32x4 *)f1w + (s * 49) * 32 + j;
        const f32x4 *av = (const f32x4 *)(act2 + s * 196);
        float acc = 0.f;
        for (int i = 0; i < 49; i++) {
            const f32x4 w = wv[i * 32], a = av[i];
            acc = __builtin_fmaf(a[0], w[0], acc);
            acc = __builtin_fmaf(a[1], w[1], acc);
            acc = __builtin_fmaf(a[2], w[2], acc);
            acc = __builtin_fmaf(a[3], w[3], acc);
        }
        part[s * 32 + j] = acc;
    }
    __syncthreads();
    if (tid < 32) {
        float h = part[tid];
        for (int s = 1; s < 8; s++) h += part[s * 32 + tid];
        hid[tid] = fmaxf(h + f1b[tid], 0.f);
    }
    __syncthreads();
    if (tid == 0) {
        float z = f2b[0];
        for (int j = 0; j < 32; j++) z = __builtin_fmaf(hid[j], f2w[j], z);
        logit[cell] = z;
    }
}

// One convolution of the blob at p: weight [cout][cin][3][3], then either its BatchNorm (gamma, beta, running mean, running var: folded by
// sv_fold_bn) or its own bias [cout].  cin == 1: conv_in's tap-K image [cout16/16][3 kk][64 lane]; else sv_pack_conv_image's.  Bias padded to
// a multiple of 16.
int pack_conv12(sv_weights_light &w, sv_conv3 &dst, const float *&p, int cout, int cin, bool has_bn)
{
    const int cout16 = (cout + 15) / 16 * 16;
    const float *cw = p;
    p += (size_t)cout * cin * 9;
    std::vector<double> k(cout);
    std::vector<float> b(cout16, 0.f);
    if (has_bn) {
        sv_fold_bn(p, p + cout, p + 2 * cout, p + 3 * cout, cout, k.data(), b.data());
        p += 4 * cout;
    } else {
        for (int oc = 0; oc < cout; oc++) b[oc] = p[oc];
        p += cout;
    }
    std::vector<float> img;
    if (cin == 1) {
        img.assign((size_t)cout16 / 16 * 3 * 64, 0.f);
        for (int oc = 0; oc < cout; oc++)
            for (int t = 0; t < 9; t++)
                img[((size_t)(oc / 16) * 3 + t / 4) * 64 + (t & 3) * 16 + (oc & 15)] = has_bn ? (float)((double)cw[oc * 9 + t] * k[oc]) : cw[oc * 9 + t];
    } else {
        img = sv_pack_conv_image(cw, has_bn ? k.data() : nullptr, cout, cin, 9);
    }
    int rc;
    if ((rc = sv_upload(w, &dst.w, img.data(), img.size()))) return rc;
    return sv_upload(w, &dst.b, b.data(), b.size());
}

}  // namespace

// blob: the state_dict of DigitCNNv3Light in key order without the num_batches_tracked entries (include/sudoku_vision_hip.h)
int svk_pack_weights_light(sv_weights_light &w, const float *blob)
{
    const float *p = blob;
    int rc;
    w.temperature = *p++;
    if ((rc = pack_conv12(w, w.conv[0], p, 24, 1, true))) return rc;
    if ((rc = pack_conv12(w, w.conv[1], p, 48, 24, true))) return rc;
    if ((rc = pack_conv12(w, w.conv[2], p, 96, 48, true))) return rc;
    std::vector<float> fcw(1280, 0.f);                       // fc.weight [10][96] -> [10][128], sv_fc2_logit's row length
    for (int j = 0; j < 10; j++)
        for (int n = 0; n < 96; n++) fcw[j * 128 + n] = p[j * 96 + n];
    p += 960;
    if ((rc = sv_upload(w, &w.fc1_w, fcw.data(), fcw.size()))) return rc;
    if ((rc = sv_upload(w, &w.fc1_b, p, 10))) return rc;
    p += 10;
    if (p - blob != SV_CNN3_LIGHT_PARAMS) return sv_fail(SV_ERR_BAD_ARG, "svk_pack_weights_light: walked %ld floats", (long)(p - blob));
    w.loaded = true;
    return SV_OK;
}

// blob: the state_dict of EmptyClassifier in key order
int svk_pack_weights_empty(sv_weights_light &w, const float *blob)
{
    const float *p = blob;
    int rc;
    if ((rc = pack_conv12(w, w.conv[0], p, 16, 1, false))) return rc;
    if ((rc = pack_conv12(w, w.conv[1], p, 32, 16, false))) return rc;
    std::vector<float> f1((size_t)32 * 1568);                // classifier.1.weight [32][1568] -> [8 s][49 i4][32 j][4 e]
    for (int j = 0; j < 32; j++)
        for (int n = 0; n < 1568; n++) f1[(((size_t)(n / 196) * 49 + (n % 196) / 4) * 32 + j) * 4 + n % 4] = p[(size_t)j * 1568 + n];
    p += 32 * 1568;
    if ((rc = sv_upload(w, &w.fc1_w, f1.data(), f1.size()))) return rc;
    if ((rc = sv_upload(w, &w.fc1_b, p, 32))) return rc;
    p += 32;
    if ((rc = sv_upload(w, &w.fc2_w, p, 32))) return rc;
    p += 32;
    if ((rc = sv_upload(w, &w.fc2_b, p, 1))) return rc;
    p += 1;
    if (p - blob != SV_EMPTY_PARAMS) return sv_fail(SV_ERR_BAD_ARG, "svk_pack_weights_empty: walked %ld floats", (long)(p - blob));
    w.loaded = true;
    return SV_OK;
}

// x: B cells, f32 [B][784] or u8 (already through preprocess_cell when that glue was asked for)
int svk_cnn3_light_forward(sv_ctx *ctx, const void *x, bool x_is_u8, long B, float *logits, float *features, u8 *digits, float *conf, hipStream_t s)
{
    const sv_weights_light &w = ctx->wl;
    auto k = x_is_u8 ? k_light<true> : k_light<false>;
    hipLaunchKernelGGL(k, dim3((unsigned)B), dim3(256), 0, s, x, (const float *)w.conv[0].w, (const float *)w.conv[0].b, (const float *)w.conv[1].w,
                       (const float *)w.conv[1].b, (const float *)w.conv[2].w, (const float *)w.conv[2].b, (const float *)w.fc1_w, (const float *)w.fc1_b,
                       w.temperature, features, logits, digits, conf);
    SV_LAUNCH_CHECK("k_light");
    return SV_OK;
}

int svk_empty_forward(sv_ctx *ctx, const void *x, bool x_is_u8, long B, float *logit, hipStream_t s)
{
    const sv_weights_light &w = ctx->we;
    auto k = x_is_u8 ? k_empty<true> : k_empty<false>;
    hipLaunchKernelGGL(k, dim3((unsigned)B), dim3(256), 0, s, x, (const float *)w.conv[0].w, (const float *)w.conv[0].b, (const float *)w.conv[1].w,
                       (const float *)w.conv[1].b, (const float *)w.fc1_w, (const float *)w.fc1_b, (const float *)w.fc2_w, (const float *)w.fc2_b, logit);
    SV_LAUNCH_CHECK("k_empty");
    return SV_OK;
}
