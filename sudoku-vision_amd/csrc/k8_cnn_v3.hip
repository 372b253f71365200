// K8 -- DigitCNNv3.forward (ml/model_v3.py:163-184, eval mode) on MI355X, true f32 throughout.
//
//   k_conv3 : every convolution of the network (stem, the ten 3x3 convs of the five ResidualBlocks, the two 1x1 stride-2 shortcuts) on the
//        f32 MFMA conv scheme of sv_conv_f32.h (input planes in LDS, K loop, weight image), BatchNorm folded into weights and bias
//        (svk_pack_weights_v3 below).  The K loop is that header's sv_conv_kloop written out in place (see there and below).  One
//        256-thread workgroup per (cell, group of NTW 16-channel output tiles) copies the cell's whole input into LDS; an M tile is 16
//        consecutive output pixels, row-major over the output plane, at the layer's stride.
//        Epilogue: + folded bias, optional ReLU, store [cell][oc][pixel].  The stem has CIN padded to 4 with three zero planes.
//   k_se_residual : the rest of a ResidualBlock (model_v3.py:33-37, :74-76) in one small kernel, one workgroup per cell: per-channel mean of
//        conv2's output (lane-strided sums + a fixed xor tree), Linear -> ReLU -> Linear -> sigmoid, then out = ReLU(t * s + shortcut).
//        Without SE the scale is skipped.
//   k_head3 : global average pool -> features[128] -> sv_head_tail (fc, argmax, temperature softmax; sv_conv_f32.h).
//
// Activations live in context scratch (sv_ctx::v3_act): three buffers of 32*784 floats per cell, rotated through the blocks, for at most
// SV_V3_SUBBATCH cells: larger batches run as consecutive sub-batches on the same stream.  A cell is always computed by the same
// instructions in the same order whatever shares its batch, so logits are batch-independent and repeatable bit for bit.
#include <cmath>
#include <cstring>
#include <vector>

#include "sv_conv_f32.h"
#include "sv_internal.h"

namespace {

constexpr int ACT = 32 * 784;            // floats per cell of one activation buffer (the largest tensor: 32 x 28 x 28)

// in: [cell][CIN_LOAD][HIN*HIN] (f32, or u8 cells taking the normalise glue), channels CIN_LOAD..CIN-1 are zero.
// wp: [COUT/16][CIN/4][KS*KS][64 lane]: lane l holds w'[oc = 16 nt + (l & 15)][ic = 4 g + (l >> 4)][tap].  out: [cell][COUT][HOUT*HOUT].
template <int CIN, int CIN_LOAD, int COUT, int HIN, int STRIDE, int KS, int MB, int NTW, bool RELU, bool U8IN>
__global__ __launch_bounds__(256) void k_conv3(const void *__restrict__ in, const float *__restrict__ wp, const float *__restrict__ bias,
                                               float *__restrict__ out)
{
    constexpr int PW = HIN + 2, PLANE = sv_conv_plane(HIN, 16), HOUT = HIN / STRIDE, HW = HOUT * HOUT, TILES = (HW + 15) / 16;
    constexpr int GROUPS = (TILES + MB - 1) / MB, TAPS = KS * KS, G4 = CIN / 4;
    static_assert(CIN % 4 == 0 && COUT % (16 * NTW) == 0 && CIN * PLANE * 4 <= 160 * 1024, "tiling");
    __shared__ float sm[CIN * PLANE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, kq = lane >> 4;
    const long cell = blockIdx.x;

    for (int i = tid; i < CIN * PLANE; i += 256) sm[i] = 0.f;
    __syncthreads();
    sv_conv_load_input<U8IN, CIN_LOAD, HIN, PLANE>(in, cell, sm, tid);
    __syncthreads();

    for (int item = wave; item < GROUPS * NTW; item += 4) {
        const int grp = item % GROUPS, nt = blockIdx.y * NTW + item / GROUPS;
        int base[MB];
#pragma unroll
        for (int i = 0; i < MB; i++) {
            int p = (grp * MB + i) * 16 + m;             // tiles past the plane recompute its last pixel; they are not stored
            p = p < HW ? p : HW - 1;
            base[i] = kq * PLANE + (p / HOUT) * STRIDE * PW + (p % HOUT) * STRIDE + (KS == 1 ? PW + 1 : 0);
        }
        f32x4 acc[MB];
#pragma unroll
        for (int i = 0; i < MB; i++) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        // sv_conv_kloop's sequence, written out: through the function the compiler no longer folds sm's address into the tap offsets and
        // the forward measures 1.5 % slower (profiles/r13_conv_f32_shared_time.txt).  A change to either copy goes into both.
        const float *wb = wp + (long)nt * G4 * TAPS * 64 + lane;
        float bcur[TAPS], bnext[TAPS];
#pragma unroll
        for (int t = 0; t < TAPS; t++) bcur[t] = wb[t * 64];
        for (int g = 0; g < G4; g++) {
            const int gn = g + 1 < G4 ? g + 1 : g;
#pragma unroll
            for (int t = 0; t < TAPS; t++) bnext[t] = wb[(gn * TAPS + t) * 64];
#pragma unroll
            for (int t = 0; t < TAPS; t++) {
#pragma unroll
                for (int i = 0; i < MB; i++) {
                    const float a = sm[base[i] + g * 4 * PLANE + (t / KS) * PW + t % KS];
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bcur[t], acc[i], 0, 0, 0);
                }
            }
#pragma unroll
            for (int t = 0; t < TAPS; t++) bcur[t] = bnext[t];
        }
        // D: column lane&15 = oc, rows 4*(lane>>4) + r = pixels
        const int oc = nt * 16 + m;
        const float bv = bias[oc];
        float *o = out + cell * (long)(COUT * HW) + (long)oc * HW;
#pragma unroll
        for (int i = 0; i < MB; i++) {
            const int p0 = (grp * MB + i) * 16 + kq * 4;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                v[r] = acc[i][r] + bv;
                if (RELU) v[r] = fmaxf(v[r], 0.f);
            }
            if (HW % 4 == 0) {
                if (p0 < HW) *(f32x4 *)(o + p0) = f32x4{v[0], v[1], v[2], v[3]};
            } else {
#pragma unroll
                for (int r = 0; r < 4; r++)
                    if (p0 + r < HW) o[p0 + r] = v[r];
            }
        }
    }
}

// t, sc, out: [cell][C][HW].  w1 [C/4][C], w2 [C][C/4] (se.excite.0 / .2), or both NULL: no SE.
template <int C, int HW>
__global__ __launch_bounds__(256) void k_se_residual(const float *__restrict__ t, const float *__restrict__ sc, const float *__restrict__ w1,
                                                     const float *__restrict__ w2, float *__restrict__ out)
{
    __shared__ float mean[C], hid[C / 4], scale[C];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long off = (long)blockIdx.x * (C * HW);
    const float *tp = t + off, *sp = sc + off;
    float *op = out + off;
    if (w1) {
        for (int c = wave; c < C; c += 4) {
            float s = 0.f;
            for (int i = lane; i < HW; i += 64) s += tp[c * HW + i];
            for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d);
            if (lane == 0) mean[c] = s / (float)HW;
        }
        __syncthreads();
        if (tid < C / 4) {
            float h = 0.f;
            for (int c = 0; c < C; c++) h = __builtin_fmaf(w1[tid * C + c], mean[c], h);
            hid[tid] = fmaxf(h, 0.f);
        }
        __syncthreads();
        if (tid < C) {
            float z = 0.f;
            for (int j = 0; j < C / 4; j++) z = __builtin_fmaf(w2[tid * (C / 4) + j], hid[j], z);
            scale[tid] = 1.f / (1.f + expf(-z));
        }
        __syncthreads();
    }
    for (int i = tid; i < C * HW; i += 256) {
        float v = tp[i];
        if (w1) v = v * scale[i / HW];
        op[i] = fmaxf(v + sp[i], 0.f);
    }
}

// x: [cell][128][49] -> features [cell][128] (or NULL), logits [cell][10], digits / conf (or NULL)
__global__ __launch_bounds__(128) void k_head3(const float *__restrict__ x, const float *__restrict__ fcw, const float *__restrict__ fcb, float temperature,
                                               float *__restrict__ features, float *__restrict__ logits, u8 *__restrict__ digits, float *__restrict__ conf)
{
    __shared__ float f[128];
    const int tid = threadIdx.x;
    const long cell = blockIdx.x;
    const float *xp = x + cell * 6272 + tid * 49;
    float s = 0.f;
    for (int i = 0; i < 49; i++) s += xp[i];
    s = s / 49.f;
    f[tid] = s;
    if (features) features[cell * 128 + tid] = s;
    sv_head_tail(f, fcw, fcb, temperature, cell, logits, digits, conf);
}

template <int CIN, int CIN_LOAD, int COUT, int HIN, int STRIDE, int KS, int MB, int NTW, bool RELU, bool U8IN>
int conv3(const void *in, const sv_conv3 &c, float *out, long n, hipStream_t s)
{
    hipLaunchKernelGGL((k_conv3<CIN, CIN_LOAD, COUT, HIN, STRIDE, KS, MB, NTW, RELU, U8IN>), dim3((unsigned)n, COUT / 16 / NTW), dim3(256), 0, s, in, c.w, c.b, out);
    SV_LAUNCH_CHECK("k_conv3");
    return SV_OK;
}

template <int C, int HW>
int se_residual(const float *t, const float *sc, const sv_weights3 &w, int layer, float *out, long n, hipStream_t s)
{
    hipLaunchKernelGGL((k_se_residual<C, HW>), dim3((unsigned)n), dim3(256), 0, s, t, sc, (const float *)w.se1[layer], (const float *)w.se2[layer], out);
    SV_LAUNCH_CHECK("k_se_residual");
    return SV_OK;
}

// conv weight [cout][cin][ks][ks] + its BatchNorm (gamma, beta, running mean, running var) at p -> k_conv3's B image and folded bias
// (sv_fold_bn, sv_pack_conv_image).  cout is a multiple of 16 here; the stem's cin = 1 is padded to 4.
int pack_conv3(sv_weights3 &w, sv_conv3 &dst, const float *&p, int cout, int cin, int ks)
{
    const int taps = ks * ks;
    const float *cw = p, *gamma = cw + (size_t)cout * cin * taps, *beta = gamma + cout, *mean = beta + cout, *var = mean + cout;
    p = var + cout;
    std::vector<double> k(cout);
    std::vector<float> b(cout);
    sv_fold_bn(gamma, beta, mean, var, cout, k.data(), b.data());
    const std::vector<float> img = sv_pack_conv_image(cw, k.data(), cout, cin, taps);
    int rc;
    if ((rc = sv_upload(w, &dst.w, img.data(), img.size()))) return rc;
    return sv_upload(w, &dst.b, b.data(), b.size());
}

}  // namespace

long svk_v3_blob_floats(bool use_se) { return use_se ? SV_CNN3_PARAMS_SE : SV_CNN3_PARAMS_NOSE; }

// blob: the state_dict of DigitCNNv3 in key order without the num_batches_tracked entries (include/sudoku_vision_hip.h)
int svk_pack_weights_v3(sv_weights3 &w, const float *blob, bool use_se)
{
    static const int CIN[5] = {32, 32, 64, 64, 128}, COUT[5] = {32, 64, 64, 128, 128};
    const float *p = blob;
    int rc;
    w.temperature = *p++;
    w.use_se = use_se;
    if ((rc = pack_conv3(w, w.stem, p, 32, 1, 3))) return rc;
    for (int l = 0; l < 5; l++) {
        const int c = COUT[l];
        if ((rc = pack_conv3(w, w.conv1[l], p, c, CIN[l], 3))) return rc;
        if ((rc = pack_conv3(w, w.conv2[l], p, c, c, 3))) return rc;
        if (use_se) {
            if ((rc = sv_upload(w, &w.se1[l], p, (size_t)c * c / 4))) return rc;
            p += c * c / 4;
            if ((rc = sv_upload(w, &w.se2[l], p, (size_t)c * c / 4))) return rc;
            p += c * c / 4;
        }
        if (CIN[l] != c && (rc = pack_conv3(w, w.shortcut[l], p, c, CIN[l], 1))) return rc;
    }
    if ((rc = sv_upload(w, &w.fc_w, p, 1280))) return rc;
    p += 1280;
    if ((rc = sv_upload(w, &w.fc_b, p, 10))) return rc;
    p += 10;
    if (p - blob != svk_v3_blob_floats(use_se)) return sv_fail(SV_ERR_BAD_ARG, "svk_pack_weights_v3: walked %ld floats", (long)(p - blob));
    w.loaded = true;
    return SV_OK;
}

size_t svk_v3_scratch_bytes(long cells)
{
    const long n = cells < SV_V3_SUBBATCH ? cells : SV_V3_SUBBATCH;
    return (size_t)n * 3 * ACT * sizeof(float);
}

// x: B cells, f32 [B][784] or u8 (already through preprocess_cell when that glue was asked for).  ctx->v3_act holds svk_v3_scratch_bytes(B).
int svk_cnn3_forward(sv_ctx *ctx, const void *x, bool x_is_u8, long B, float *logits, float *features, u8 *digits, float *conf, hipStream_t s)
{
    const sv_weights3 &w = ctx->w3;
    const long cap = ctx->v3_cells;
    float *P = ctx->v3_act.as<float>(), *Q = P + cap * ACT, *R = Q + cap * ACT;
    float *P2 = P + cap * (ACT / 2), *Q2 = Q + cap * (ACT / 2);      // second halves: the stride-2 blocks hold two tensors in one buffer
    const auto stem = x_is_u8 ? conv3<4, 1, 32, 28, 1, 3, 7, 1, true, true> : conv3<4, 1, 32, 28, 1, 3, 7, 1, true, false>;
    const size_t cell_bytes = 784 * (x_is_u8 ? sizeof(u8) : sizeof(float));
    int rc;
    for (long b0 = 0; b0 < B; b0 += SV_V3_SUBBATCH) {
        const long n = B - b0 < SV_V3_SUBBATCH ? B - b0 : SV_V3_SUBBATCH;
        if ((rc = stem((const char *)x + b0 * cell_bytes, w.stem, P, n, s))) return rc;
        // layer1: 32 -> 32, 28x28
        if ((rc = conv3<32, 32, 32, 28, 1, 3, 7, 1, true, false>(P, w.conv1[0], Q, n, s))) return rc;
        if ((rc = conv3<32, 32, 32, 28, 1, 3, 7, 1, false, false>(Q, w.conv2[0], R, n, s))) return rc;
        if ((rc = se_residual<32, 784>(R, P, w, 0, Q, n, s))) return rc;
        // layer2: 32 -> 64, stride 2 -> 14x14
        if ((rc = conv3<32, 32, 64, 28, 2, 1, 7, 2, false, false>(Q, w.shortcut[1], P, n, s))) return rc;
        if ((rc = conv3<32, 32, 64, 28, 2, 3, 7, 2, true, false>(Q, w.conv1[1], R, n, s))) return rc;
        if ((rc = conv3<64, 64, 64, 14, 1, 3, 7, 2, false, false>(R, w.conv2[1], P2, n, s))) return rc;
        if ((rc = se_residual<64, 196>(P2, P, w, 1, R, n, s))) return rc;
        // layer3: 64 -> 64
        if ((rc = conv3<64, 64, 64, 14, 1, 3, 7, 2, true, false>(R, w.conv1[2], P, n, s))) return rc;
        if ((rc = conv3<64, 64, 64, 14, 1, 3, 7, 2, false, false>(P, w.conv2[2], Q, n, s))) return rc;
        if ((rc = se_residual<64, 196>(Q, R, w, 2, P, n, s))) return rc;
        // layer4: 64 -> 128, stride 2 -> 7x7
        if ((rc = conv3<64, 64, 128, 14, 2, 1, 4, 4, false, false>(P, w.shortcut[3], Q, n, s))) return rc;
        if ((rc = conv3<64, 64, 128, 14, 2, 3, 4, 4, true, false>(P, w.conv1[3], R, n, s))) return rc;
        if ((rc = conv3<128, 128, 128, 7, 1, 3, 4, 4, false, false>(R, w.conv2[3], Q2, n, s))) return rc;
        if ((rc = se_residual<128, 49>(Q2, Q, w, 3, R, n, s))) return rc;
        // layer5: 128 -> 128
        if ((rc = conv3<128, 128, 128, 7, 1, 3, 4, 4, true, false>(R, w.conv1[4], P, n, s))) return rc;
        if ((rc = conv3<128, 128, 128, 7, 1, 3, 4, 4, false, false>(P, w.conv2[4], Q, n, s))) return rc;
        if ((rc = se_residual<128, 49>(Q, R, w, 4, P, n, s))) return rc;
        hipLaunchKernelGGL(k_head3, dim3((unsigned)n), dim3(128), 0, s, (const float *)P, (const float *)w.fc_w, (const float *)w.fc_b, w.temperature,
                           features ? features + b0 * 128 : nullptr, logits + b0 * 10, digits ? digits + b0 : nullptr, conf ? conf + b0 : nullptr);
        SV_LAUNCH_CHECK("k_head3");
    }
    return SV_OK;
}
