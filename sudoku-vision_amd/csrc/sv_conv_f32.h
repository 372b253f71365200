// The f32 convolution core that K8 (k8_cnn_v3.hip) and K12 (k12_cnn_v3_light.hip) share: what carries their bit-for-bit claim is stated
// here (k_conv3 repeats the K loop in place, see sv_conv_kloop).
//
// A convolution is an implicit GEMM on v_mfma_f32_16x16x4_f32.  The workgroup holds a cell's input in LDS as zero-bordered planes
// [ic][PLANE]; M = 16 output pixels, N = 16 output channels, K = 4 input channels of one tap per instruction.  A is one ds_read_b32 per
// lane (pixel lane & 15, channel lane >> 4) at base + the tap's offset, B one coalesced global dword per lane from an image packed on the
// host (sv_pack_conv_image), loaded one 4-channel group ahead.  A wave keeps MB M-tiles of one N-tile in MB independent accumulators, so
// each B value feeds MB MFMAs.  The K order of every output (ic groups outer, taps inner) is fixed here and depends on nothing else, the
// batch least of all.  Which pixels a tile holds (base[]) and where the result goes (the epilogue) are the caller's.
// The head tail (fc -> argmax -> temperature softmax) and the host side of the weights (BatchNorm fold, B image) are here as well.
#pragma once
#include <cmath>
#include <vector>

#include "sv_device.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// LDS row of one input channel: the zero-bordered (hin+2)^2 plane rounded up to `residue` mod 32 floats.  16: the four ic rows a
// ds_read_b32 touches fall on different banks.  8: the input of a layer with the 2x2 max pool in its epilogue, whose M tile is four 2x2
// windows; 8 puts the windows of lanes 0..31 on 32 different banks.
constexpr int sv_conv_plane(int hin, int residue) { return (((hin + 2) * (hin + 2) - residue + 31) / 32) * 32 + residue; }

// in: [cell][CIN_LOAD][HIN*HIN] (f32, or u8 cells taking the normalise glue) -> the interiors of sm's first CIN_LOAD planes.  The caller
// zeroed sm (borders, and the planes of a CIN padded beyond CIN_LOAD) and has a barrier on either side.
template <bool U8IN, int CIN_LOAD, int HIN, int PLANE>
__device__ __forceinline__ void sv_conv_load_input(const void *in, long cell, float *sm, int tid)
{
    constexpr int PW = HIN + 2, NIN = CIN_LOAD * HIN * HIN;
    for (int i = tid; i < NIN; i += 256) {
        const int c = i / (HIN * HIN), p = i % (HIN * HIN);
        float v;
        if (U8IN) v = sv_glue_norm(((const u8 *)in)[cell * NIN + i]);
        else v = ((const float *)in)[cell * NIN + i];
        sm[c * PLANE + (p / HIN + 1) * PW + p % HIN + 1] = v;
    }
}

// The K loop of one wave's MB tiles: acc[i] += sum over g < G4, t < KS*KS of A(base[i] + g 4 PLANE + tap t) * B(g, t), in that order.
// sm: the input planes (row PW floats).  base[i]: lane's address of tile i's pixel at tap 0, channel lane >> 4.  wb: the lane's dword of the
// N-tile's B image [G4][KS*KS][64 lane].  The last group prefetches itself again, so no load leaves the image.
// k_conv3 (k8_cnn_v3.hip) carries this loop written out, statement for statement: with sm a __shared__ array of the kernel itself the
// compiler folds its address into the tap offsets, which it does not do through a pointer parameter, and K8 measures 1.5 % faster so.
template <int G4, int KS, int PW, int PLANE, int MB>
__device__ __forceinline__ void sv_conv_kloop(const float *sm, const int (&base)[MB], const float *wb, f32x4 (&acc)[MB])
{
    constexpr int TAPS = KS * KS;
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
}

// The tail of a digit head, called by every thread of the workgroup once f is written: f (LDS, 128 features, zero beyond the model's own)
// -> logits [cell][10] through sv_fc2_logit (fcw [10][128]), then digits / conf (or NULL) by sv_digit_conf_t.
__device__ __forceinline__ void sv_head_tail(const float *f, const float *__restrict__ fcw, const float *__restrict__ fcb, float temperature, long cell,
                                             float *__restrict__ logits, u8 *__restrict__ digits, float *__restrict__ conf)
{
    __shared__ float lg[10];
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < 10) {
        lg[tid] = sv_fc2_logit(f, (const float(*)[128])fcw, fcb, tid);
        logits[cell * 10 + tid] = lg[tid];
    }
    __syncthreads();
    if (tid == 0) sv_digit_conf_t(lg, temperature, cell, digits, conf);
}

// ---- host side ----
// BatchNorm (gamma, beta, running mean, running var, each [cout]) as a scale and a bias, in float64: k = gamma / sqrt(var + eps),
// b' = beta - mean * k rounded once, eps = 1e-5 (nn.BatchNorm2d)
inline void sv_fold_bn(const float *gamma, const float *beta, const float *mean, const float *var, int cout, double *k, float *b)
{
    for (int oc = 0; oc < cout; oc++) {
        k[oc] = (double)gamma[oc] / std::sqrt((double)var[oc] + 1e-5);
        b[oc] = (float)((double)beta[oc] - (double)mean[oc] * k[oc]);
    }
}

// conv weight cw [cout][cin][taps] -> sv_conv_kloop's B image [cout16/16][cin4/4][taps][64 lane], cout padded to a multiple of 16 and cin to
// a multiple of 4 with zeros: lane l holds w'[oc = 16 nt + (l & 15)][ic = 4 g + (l >> 4)][tap], w' = w * k[oc] in float64 rounded once
// (k from sv_fold_bn), or w itself when k is NULL.
inline std::vector<float> sv_pack_conv_image(const float *cw, const double *k, int cout, int cin, int taps)
{
    const int g4 = (cin + 3) / 4;
    std::vector<float> img((size_t)((cout + 15) / 16) * g4 * taps * 64, 0.f);
    for (int oc = 0; oc < cout; oc++)
        for (int ic = 0; ic < cin; ic++)
            for (int t = 0; t < taps; t++) {
                const float v = cw[((size_t)oc * cin + ic) * taps + t];
                img[(((size_t)(oc / 16) * g4 + ic / 4) * taps + t) * 64 + (ic & 3) * 16 + (oc & 15)] = k ? (float)((double)v * k[oc]) : v;
            }
    return img;
}
