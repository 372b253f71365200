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
//
// MC dropout (forward_with_uncertainty, ml/model_v3.py:186-214; svk_cnn3_forward_mc at the end): the same launches with the three dropouts
// of :167, :170 and :181 active and BatchNorm on its running statistics.  k_mc_masks, k_mc_expand, k_head3_mc and k_mc_reduce are its
// own; layer3's mask is k_se_residual's MASK flag; the masks come from sv_philox.h.
#include <cmath>
#include <cstring>
#include <vector>

#include "sv_conv_f32.h"
#include "sv_internal.h"
#include "sv_philox.h"

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
// MASK (the MC forward's layer3): spatial dropout on the block's output, out = keep ? out / q : 0 with q = 1 - p, keep the cell's bytes
// of site 1 in the chunk's mask rows (k_mc_masks).  q = 1 and all kept is the unmasked result bit for bit.
template <int C, int HW, bool MASK>
__global__ __launch_bounds__(256) void k_se_residual(const float *__restrict__ t, const float *__restrict__ sc, const float *__restrict__ w1,
                                                     const float *__restrict__ w2, float *__restrict__ out, const u8 *__restrict__ keep, float q)
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
        v = fmaxf(v + sp[i], 0.f);
        if (MASK) v = keep[(long)blockIdx.x * SV_MC_MASK + sv_mc_site_offset(1) + i / HW] ? v / q : 0.f;
        op[i] = v;
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

// ---- MC dropout (forward_with_uncertainty, ml/model_v3.py:186-214): the kernels around the forward's own ----
// A chunk is nc whole cells b0 .. b0 + nc - 1 with all S samples of each: expanded index e = (b - b0) * S + s, ne = nc * S of them.

// The chunk's keep bytes m [ne][SV_MC_MASK] (1 = keep; site 0, 1, 2 one after the other): from the caller's in1/in3/inf
// (u8 [S][B][32 / 64 / 128], nonzero = keep) when in1 is there, else from sv_mc_draw.  out1/out3/outf (same shapes, each or NULL) receive
// them.  One thread per (e, group of four channels): 8 + 16 + 32 groups per e.
__global__ __launch_bounds__(256) void k_mc_masks(unsigned long long seed, unsigned long long offset, unsigned long long thr_sp, unsigned long long thr_fc,
                                                  const u8 *__restrict__ in1, const u8 *__restrict__ in3, const u8 *__restrict__ inf, long B, int S, long b0,
                                                  long ne, u8 *__restrict__ m, u8 *__restrict__ out1, u8 *__restrict__ out3, u8 *__restrict__ outf)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= ne * (SV_MC_MASK / 4)) return;
    const long e = idx / (SV_MC_MASK / 4);
    const int q = (int)(idx % (SV_MC_MASK / 4)), site = q < 8 ? 0 : q < 24 ? 1 : 2, g = q - sv_mc_site_offset(site) / 4, C = sv_mc_channels(site);
    const long b = b0 + e / S;
    const int s = (int)(e % S);
    const long at = ((long)s * B + b) * C + 4 * g;
    const u8 *in = site == 0 ? in1 : site == 1 ? in3 : inf;
    u8 *out = site == 0 ? out1 : site == 1 ? out3 : outf;
    u8 k[4];
    if (in1) {
#pragma unroll
        for (int r = 0; r < 4; r++) k[r] = in[at + r] != 0;
    } else {
        const sv_philox4 w = sv_mc_draw(seed, offset, (uint32_t)s, (uint32_t)b, site, g);
        const unsigned long long thr = site == 2 ? thr_fc : thr_sp;
#pragma unroll
        for (int r = 0; r < 4; r++) k[r] = (unsigned long long)w.v[r] < thr;
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        m[e * SV_MC_MASK + 4 * q + r] = k[r];
        if (out) out[at + r] = k[r];
    }
}

// layer1's output of the chunk's cells l1 [nc][32][784] -> the S masked copies out [ne][32][784] that layer2 reads:
// out = keep ? l1 / q : 0 (q = 1 - p; site 0 of m).  Four pixels of one channel per thread and step.
__global__ __launch_bounds__(256) void k_mc_expand(const float *__restrict__ l1, const u8 *__restrict__ m, float q, int S, float *__restrict__ out)
{
    const long e = blockIdx.x;
    const f32x4 *src = (const f32x4 *)(l1 + (e / S) * ACT);
    f32x4 *dst = (f32x4 *)(out + e * ACT);
    for (int i = threadIdx.x; i < ACT / 4; i += 256) {
        const f32x4 v = src[i];
        const bool keep = m[e * SV_MC_MASK + i / 196];
        dst[i] = keep ? f32x4{v[0] / q, v[1] / q, v[2] / q, v[3] / q} : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// k_head3 per (sample, cell) e: global average pool -> feature dropout (keep ? f / q : 0, q = 1 - p, site 2 of m) -> fc by the same
// sv_fc2_logit on the same LDS features as sv_head_tail -> logits_out [S][B][10] (or NULL) -> probs [ne][10] = softmax(logits / temperature)
__global__ __launch_bounds__(128) void k_head3_mc(const float *__restrict__ x, const float *__restrict__ fcw, const float *__restrict__ fcb, float temperature,
                                                  const u8 *__restrict__ m, float q, long B, int S, long b0, float *__restrict__ logits_out,
                                                  float *__restrict__ probs)
{
    __shared__ float f[128], lg[10];
    const int tid = threadIdx.x;
    const long e = blockIdx.x;
    const float *xp = x + e * 6272 + tid * 49;
    float s = 0.f;
    for (int i = 0; i < 49; i++) s += xp[i];
    s = s / 49.f;
    f[tid] = m[e * SV_MC_MASK + sv_mc_site_offset(2) + tid] ? s / q : 0.f;
    __syncthreads();
    if (tid < 10) {
        lg[tid] = sv_fc2_logit(f, (const float(*)[128])fcw, fcb, tid);
        if (logits_out) logits_out[((e % S) * B + b0 + e / S) * 10 + tid] = lg[tid];
    }
    __syncthreads();
    if (tid == 0) {
        float z[10], best;
        for (int j = 0; j < 10; j++) z[j] = lg[j] / temperature;
        sv_argmax10(z, best);
        float den = 0.f;
        for (int j = 0; j < 10; j++) den += (z[j] = expf(z[j] - best));
        for (int j = 0; j < 10; j++) probs[e * 10 + j] = z[j] / den;
    }
}

// probs [nc][S][10] -> per cell: mean over the samples in ascending order (summed in double, rounded once), the unbiased two-pass standard
// deviation sqrt(sum (p - mean)^2 / (S - 1)) in f32 (S = 1: 0 / 0 = NaN, as torch.std), the first maximum of the mean.  Equal samples
// give that value as the mean and a deviation of exactly 0.  mean, std [nc][10], predicted [nc]: the chunk's rows, each or NULL.
__global__ __launch_bounds__(64) void k_mc_reduce(const float *__restrict__ probs, int S, long nc, float *__restrict__ mean, float *__restrict__ std,
                                                  long long *__restrict__ predicted)
{
    const long j = (long)blockIdx.x * 64 + threadIdx.x;
    if (j >= nc) return;
    const float *p = probs + j * S * 10;
    float mu[10];
    for (int c = 0; c < 10; c++) {
        double a = 0.0;
        for (int s = 0; s < S; s++) a += (double)p[s * 10 + c];
        mu[c] = (float)(a / (double)S);
        if (mean) mean[j * 10 + c] = mu[c];
        if (std) {
            float ss = 0.f;
            for (int s = 0; s < S; s++) {
                const float d = p[s * 10 + c] - mu[c];
                ss += d * d;
            }
            std[j * 10 + c] = sqrtf(ss / (float)(S - 1));
        }
    }
    float best;
    if (predicted) predicted[j] = sv_argmax10(mu, best);
}

template <int CIN, int CIN_LOAD, int COUT, int HIN, int STRIDE, int KS, int MB, int NTW, bool RELU, bool U8IN>
int conv3(const void *in, const sv_conv3 &c, float *out, long n, hipStream_t s)
{
    hipLaunchKernelGGL((k_conv3<CIN, CIN_LOAD, COUT, HIN, STRIDE, KS, MB, NTW, RELU, U8IN>), dim3((unsigned)n, COUT / 16 / NTW), dim3(256), 0, s, in, c.w, c.b, out);
    SV_LAUNCH_CHECK("k_conv3");
    return SV_OK;
}

// keep: the chunk's mask rows of an MC forward (then the block's output takes spatial dropout at q = 1 - p), or NULL
template <int C, int HW>
int se_residual(const float *t, const float *sc, const sv_weights3 &w, int layer, float *out, long n, hipStream_t s, const u8 *keep = nullptr, float q = 1.f)
{
    const float *w1 = w.se1[layer], *w2 = w.se2[layer];
    if (keep) hipLaunchKernelGGL((k_se_residual<C, HW, true>), dim3((unsigned)n), dim3(256), 0, s, t, sc, w1, w2, out, keep, q);
    else hipLaunchKernelGGL((k_se_residual<C, HW, false>), dim3((unsigned)n), dim3(256), 0, s, t, sc, w1, w2, out, keep, q);
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

// The MC forward's own scratch (sv_ctx::v3_mc), a constant: layer1's output of a chunk's cells [SV_V3_SUBBATCH][32*784] f32 (S = 1 has that
// many cells in a chunk), the chunk's probabilities [SV_V3_SUBBATCH][10] f32, its keep bytes [SV_V3_SUBBATCH][SV_MC_MASK].
size_t svk_v3_mc_scratch_bytes() { return (size_t)SV_V3_SUBBATCH * (ACT * sizeof(float) + 10 * sizeof(float) + SV_MC_MASK); }

namespace {

// The three activation buffers of ctx->v3_act; P2 / Q2: second halves, the stride-2 blocks hold two tensors in one buffer
struct v3_bufs {
    float *P, *Q, *R, *P2, *Q2;
    explicit v3_bufs(const sv_ctx *ctx) : P(ctx->v3_act.as<float>()), Q(P + ctx->v3_cells * ACT), R(Q + ctx->v3_cells * ACT), P2(P + ctx->v3_cells * (ACT / 2)), Q2(Q + ctx->v3_cells * (ACT / 2)) {}
};

// stem + layer1 of n cells x (f32 [n][784] or u8) -> l1 [n][32][784], which is a.Q or a buffer outside a (P and R are used up)
int v3_front(const sv_weights3 &w, const v3_bufs &a, const void *x, bool x_is_u8, float *l1, long n, hipStream_t s)
{
    const auto stem = x_is_u8 ? conv3<4, 1, 32, 28, 1, 3, 7, 1, true, true> : conv3<4, 1, 32, 28, 1, 3, 7, 1, true, false>;
    int rc;
    if ((rc = stem(x, w.stem, a.P, n, s))) return rc;
    // layer1: 32 -> 32, 28x28
    if ((rc = conv3<32, 32, 32, 28, 1, 3, 7, 1, true, false>(a.P, w.conv1[0], a.Q, n, s))) return rc;
    if ((rc = conv3<32, 32, 32, 28, 1, 3, 7, 1, false, false>(a.Q, w.conv2[0], a.R, n, s))) return rc;
    return se_residual<32, 784>(a.R, a.P, w, 0, l1, n, s);
}

// layers 2..5 of n cells: a.Q [n][32][784] -> a.P [n][128][49].  keep, q3: an MC forward's mask rows and 1 - p for layer3's output, or NULL
int v3_back(const sv_weights3 &w, const v3_bufs &a, long n, hipStream_t s, const u8 *keep = nullptr, float q3 = 1.f)
{
    float *const P = a.P, *const Q = a.Q, *const R = a.R, *const P2 = a.P2, *const Q2 = a.Q2;
    int rc;
    // layer2: 32 -> 64, stride 2 -> 14x14
    if ((rc = conv3<32, 32, 64, 28, 2, 1, 7, 2, false, false>(Q, w.shortcut[1], P, n, s))) return rc;
    if ((rc = conv3<32, 32, 64, 28, 2, 3, 7, 2, true, false>(Q, w.conv1[1], R, n, s))) return rc;
    if ((rc = conv3<64, 64, 64, 14, 1, 3, 7, 2, false, false>(R, w.conv2[1], P2, n, s))) return rc;
    if ((rc = se_residual<64, 196>(P2, P, w, 1, R, n, s))) return rc;
    // layer3: 64 -> 64
    if ((rc = conv3<64, 64, 64, 14, 1, 3, 7, 2, true, false>(R, w.conv1[2], P, n, s))) return rc;
    if ((rc = conv3<64, 64, 64, 14, 1, 3, 7, 2, false, false>(P, w.conv2[2], Q, n, s))) return rc;
    if ((rc = se_residual<64, 196>(Q, R, w, 2, P, n, s, keep, q3))) return rc;
    // layer4: 64 -> 128, stride 2 -> 7x7
    if ((rc = conv3<64, 64, 128, 14, 2, 1, 4, 4, false, false>(P, w.shortcut[3], Q, n, s))) return rc;
    if ((rc = conv3<64, 64, 128, 14, 2, 3, 4, 4, true, false>(P, w.conv1[3], R, n, s))) return rc;
    if ((rc = conv3<128, 128, 128, 7, 1, 3, 4, 4, false, false>(R, w.conv2[3], Q2, n, s))) return rc;
    if ((rc = se_residual<128, 49>(Q2, Q, w, 3, R, n, s))) return rc;
    // layer5: 128 -> 128
    if ((rc = conv3<128, 128, 128, 7, 1, 3, 4, 4, true, false>(R, w.conv1[4], P, n, s))) return rc;
    if ((rc = conv3<128, 128, 128, 7, 1, 3, 4, 4, false, false>(P, w.conv2[4], Q, n, s))) return rc;
    return se_residual<128, 49>(Q, R, w, 4, P, n, s);
}

}  // namespace

// x: B cells, f32 [B][784] or u8 (already through preprocess_cell when that glue was asked for).  ctx->v3_act holds svk_v3_scratch_bytes(B).
int svk_cnn3_forward(sv_ctx *ctx, const void *x, bool x_is_u8, long B, float *logits, float *features, u8 *digits, float *conf, hipStream_t s)
{
    const sv_weights3 &w = ctx->w3;
    const v3_bufs a(ctx);
    const size_t cell_bytes = 784 * (x_is_u8 ? sizeof(u8) : sizeof(float));
    int rc;
    for (long b0 = 0; b0 < B; b0 += SV_V3_SUBBATCH) {
        const long n = B - b0 < SV_V3_SUBBATCH ? B - b0 : SV_V3_SUBBATCH;
        if ((rc = v3_front(w, a, (const char *)x + b0 * cell_bytes, x_is_u8, a.Q, n, s))) return rc;
        if ((rc = v3_back(w, a, n, s))) return rc;
        hipLaunchKernelGGL(k_head3, dim3((unsigned)n), dim3(128), 0, s, (const float *)a.P, (const float *)w.fc_w, (const float *)w.fc_b, w.temperature,
                           features ? features + b0 * 128 : nullptr, logits + b0 * 10, digits ? digits + b0 : nullptr, conf ? conf + b0 : nullptr);
        SV_LAUNCH_CHECK("k_head3");
    }
    return SV_OK;
}

// The MC-dropout forward (sv_cnn3_forward_mc_f32): x f32 [B][784], S samples per cell.  ctx->v3_act holds SV_V3_SUBBATCH cells and ctx->v3_mc
// svk_v3_mc_scratch_bytes().  The batch goes through in chunks of SV_V3_SUBBATCH / S whole cells, at most SV_V3_SUBBATCH (sample, cell)
// pairs at a time: stem and layer1 once per cell, then the masked copies of layer1's output through layers 2..5 with the launches of
// svk_cnn3_forward (a pair takes the MFMA sequence of an eval forward, whatever shares its chunk), the masked head, the reduction.
// keep_in: all three or none.
int svk_cnn3_forward_mc(sv_ctx *ctx, const float *x, long B, int S, float p_spatial, float p_fc, uint64_t seed, uint64_t offset, const u8 *const keep_in[3],
                        float *mean, float *std, long long *predicted, float *logits_out, u8 *const keep_out[3], hipStream_t s)
{
    const sv_weights3 &w = ctx->w3;
    const v3_bufs a(ctx);
    float *const l1 = ctx->v3_mc.as<float>(), *const probs = l1 + (size_t)SV_V3_SUBBATCH * ACT;
    u8 *const m = (u8 *)(probs + SV_V3_SUBBATCH * 10);
    const float q_sp = 1.f - p_spatial, q_fc = 1.f - p_fc;
    const unsigned long long thr_sp = sv_mc_keep_threshold(p_spatial), thr_fc = sv_mc_keep_threshold(p_fc);
    const long per = SV_V3_SUBBATCH / S;
    int rc;
    for (long b0 = 0; b0 < B; b0 += per) {
        const long nc = B - b0 < per ? B - b0 : per, ne = nc * S;
        hipLaunchKernelGGL(k_mc_masks, dim3((unsigned)((ne * (SV_MC_MASK / 4) + 255) / 256)), dim3(256), 0, s, (unsigned long long)seed, (unsigned long long)offset,
                           thr_sp, thr_fc, keep_in[0], keep_in[1], keep_in[2], B, S, b0, ne, m, keep_out[0], keep_out[1], keep_out[2]);
        SV_LAUNCH_CHECK("k_mc_masks");
        if ((rc = v3_front(w, a, x + b0 * 784, false, l1, nc, s))) return rc;
        hipLaunchKernelGGL(k_mc_expand, dim3((unsigned)ne), dim3(256), 0, s, (const float *)l1, (const u8 *)m, q_sp, S, a.Q);
        SV_LAUNCH_CHECK("k_mc_expand");
        if ((rc = v3_back(w, a, ne, s, m, q_sp))) return rc;
        hipLaunchKernelGGL(k_head3_mc, dim3((unsigned)ne), dim3(128), 0, s, (const float *)a.P, (const float *)w.fc_w, (const float *)w.fc_b, w.temperature,
                           (const u8 *)m, q_fc, B, S, b0, logits_out, probs);
        SV_LAUNCH_CHECK("k_head3_mc");
        if (mean || std || predicted) {
            hipLaunchKernelGGL(k_mc_reduce, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, s, (const float *)probs, S, nc, mean ? mean + b0 * 10 : nullptr,
                               std ? std + b0 * 10 : nullptr, predicted ? predicted + b0 : nullptr);
            SV_LAUNCH_CHECK("k_mc_reduce");
        }
    }
    return SV_OK;
}
