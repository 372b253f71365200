// The step bodies of K22 (k22_augment.hip) and of K23's phase B (k23_synth_cells.hip): one text, included by both kernels.
// include/sudoku_vision_hip.h states the arithmetic of every step; both files are compiled with -ffp-contract=off.
#pragma once
#include "sv_device.h"
#include "sv_internal.h"
#include "sv_philox.h"

namespace {

struct AugShared {
    sv_aug_step st;
    double M[9];
    unsigned sum;
};

__device__ __forceinline__ u8 aug_clip_trunc(double v) { return (u8)(int)fmin(fmax(v, 0.0), 255.0); }

// one pixel of cv2.resize(in, (nw, nh)) at (x, y) of the scaled image
__device__ __forceinline__ int aug_resize_px(const u8 *in, int H, int W, int nh, int nw, int x, int y)
{
    int xo, a0, a1, yo, b0, b1;
    sv_resize_axis(W, nw, x, xo, a0, a1);
    sv_resize_axis(H, nh, y, yo, b0, b1);
    return sv_resize_px(xo, a0, a1, yo, b0, b1, H, W, [=](int tx, int ty) { return (int)in[ty * W + tx]; });
}

// one separable pass of the elastic step's Gaussian along x (dx = 1) or y (dx = 0): taps t[0..r] by distance, REFLECT_101,
// accumulated from -r to +r
__device__ __forceinline__ void aug_field_pass(const float *in, float *out, int H, int W, const float *t, int r, bool along_x, int tid)
{
    for (int p = tid; p < H * W; p += 256) {
        const int y = p / W, x = p - y * W;
        float acc = 0.f;
        for (int j = -r; j <= r; j++) {
            const int q = along_x ? y * W + sv_reflect101(x + j, W) : sv_reflect101(y + j, H) * W + x;
            const float term = __fmul_rn(t[j < 0 ? -j : j], in[q]);
            acc = j == -r ? term : __fadd_rn(acc, term);
        }
        out[p] = acc;
    }
}

// One of K22's eleven step kinds, `op` with its arguments in sh.st, from plane `in` to plane `out` by the 256 threads of the workgroup; fx,
// fy, ft are the three f32 planes of the elastic step.  border is the warps' border (sv_remap_sample; K22: -1), pad the value the scale
// step pads with (K22: 128).  Returns whether `out` was written (the same for every thread: st is uniform); an op it does not
// know is the identity.  The caller has put a barrier between the write of sh.st / sh.sum = 0 and this call.
__device__ __forceinline__ bool aug_run_step(AugShared &sh, int op, int border, int pad, const u8 *in, u8 *out, int H, int W, float *fx, float *fy, float *ft, uint64_t seed, uint64_t g, int slot, int tid)
{
    const int HW = H * W;
    const sv_aug_step &st = sh.st;
    const uint32_t salt = (uint32_t)st.i[4];
    bool wrote = true;
    switch (op) {
    case SV_AUG_AFFINE: {
        if (tid == 0) sv_affine_invert(st.d, sh.M);
        __syncthreads();
        for (int p = tid; p < HW; p += 256) {
            const int y = p / W, x = p - y * W;
            int X, Y, sx, sy, a, b;
            sv_affine_coord(sh.M, x, y, X, Y);
            sv_remap_split(X, Y, sx, sy, a, b);
            out[p] = (u8)sv_remap_sample(in, H, W, W, sx, sy, a, b, border);
        }
        break;
    }
    case SV_AUG_PERSPECTIVE: {
        if (tid == 0) {
            // cv::invert of a 3x3: cofactors times 1/det; a singular matrix gives zeros
            const double *S = st.d;
            auto cof = [](double a, double b, double c, double d) { return __dsub_rn(__dmul_rn(a, b), __dmul_rn(c, d)); };
            const double c0 = cof(S[4], S[8], S[5], S[7]), c1 = cof(S[3], S[8], S[5], S[6]), c2 = cof(S[3], S[7], S[4], S[6]);
            double det = __dadd_rn(__dsub_rn(__dmul_rn(S[0], c0), __dmul_rn(S[1], c1)), __dmul_rn(S[2], c2));
            det = det != 0.0 ? __ddiv_rn(1.0, det) : 0.0;
            sh.M[0] = __dmul_rn(c0, det);
            sh.M[1] = __dmul_rn(cof(S[2], S[7], S[1], S[8]), det);
            sh.M[2] = __dmul_rn(cof(S[1], S[5], S[2], S[4]), det);
            sh.M[3] = __dmul_rn(cof(S[5], S[6], S[3], S[8]), det);
            sh.M[4] = __dmul_rn(cof(S[0], S[8], S[2], S[6]), det);
            sh.M[5] = __dmul_rn(cof(S[2], S[3], S[0], S[5]), det);
            sh.M[6] = __dmul_rn(c2, det);
            sh.M[7] = __dmul_rn(cof(S[1], S[6], S[0], S[7]), det);
            sh.M[8] = __dmul_rn(cof(S[0], S[4], S[1], S[3]), det);
        }
        __syncthreads();
        for (int p = tid; p < HW; p += 256) {
            const int y = p / W, x = p - y * W;
            int sx, sy, a, b;
            sv_warp_coord(sh.M, x, y, W, sx, sy, a, b);       // W <= 64: the image is one block of cv2's, its origin column 0
            out[p] = (u8)sv_remap_sample(in, H, W, W, sx, sy, a, b, border);
        }
        break;
    }
    case SV_AUG_BRIGHTNESS: {
        const float delta = (float)st.d[0];
        for (int p = tid; p < HW; p += 256) out[p] = (u8)(int)fminf(fmaxf(__fadd_rn((float)in[p], delta), 0.f), 255.f);
        break;
    }
    case SV_AUG_CONTRAST: {
        unsigned part = 0;
        for (int p = tid; p < HW; p += 256) part += in[p];
        atomicAdd(&sh.sum, part);                          // integers: exact in any order
        __syncthreads();
        const double mean = __ddiv_rn((double)sh.sum, (double)HW), factor = st.d[0];
        for (int p = tid; p < HW; p += 256) out[p] = aug_clip_trunc(__dadd_rn(__dmul_rn(__dsub_rn((double)in[p], mean), factor), mean));
        break;
    }
    case SV_AUG_BLUR: {
        const int k = st.i[0];
        if (k != 3 && k != 5) { wrote = false; break; }
        const int r = k >> 1;
        for (int p = tid; p < HW; p += 256) {
            const int y = p / W, x = p - y * W;
            unsigned acc = 0;
            for (int j = -r; j <= r; j++) {
                const u8 *row = in + sv_reflect101(y + j, H) * W;
                unsigned h = 0;
                for (int i = -r; i <= r; i++) {
                    const unsigned ti = k == 3 ? (i == 0 ? 2u : 1u) : (i == 0 ? 6u : (i == 1 || i == -1) ? 4u : 1u);
                    h += ti * row[sv_reflect101(x + i, W)];
                }
                const unsigned tj = k == 3 ? (j == 0 ? 2u : 1u) : (j == 0 ? 6u : (j == 1 || j == -1) ? 4u : 1u);
                acc += tj * h;
            }
            out[p] = (u8)(k == 3 ? (acc + 8u) >> 4 : (acc + 128u) >> 8);
        }
        break;
    }
    case SV_AUG_SCALE: {
        const int nw = sv_clamp(st.i[0], 1, 2 * SV_AUG_MAX_SIDE), nh = sv_clamp(st.i[1], 1, 2 * SV_AUG_MAX_SIDE);
        // floor divisions, as Python's //
        const int oy = st.i[2] ? (nh - H) >> 1 : -((H - nh) >> 1), ox = st.i[2] ? (nw - W) >> 1 : -((W - nw) >> 1);
        for (int p = tid; p < HW; p += 256) {
            const int y = p / W + oy, x = p % W + ox;
            out[p] = ((unsigned)x < (unsigned)nw && (unsigned)y < (unsigned)nh) ? (u8)aug_resize_px(in, H, W, nh, nw, x, y) : (u8)pad;
        }
        break;
    }
    case SV_AUG_FILL_RECT: {
        const long x0 = st.i[0], y0 = st.i[1], x1 = x0 + st.i[2], y1 = y0 + st.i[3];
        for (int p = tid; p < HW; p += 256) {
            const int y = p / W, x = p - y * W;
            out[p] = (x >= x0 && x < x1 && y >= y0 && y < y1) ? (u8)st.i[4] : in[p];
        }
        break;
    }
    case SV_AUG_ELASTIC: {
        const int r = st.i[0];
        if (r < 0 || r > SV_AUG_MAX_RADIUS) { wrote = false; break; }
        for (int p = tid; p < HW; p += 256) {
            const sv_philox4 w = sv_aug_draw(seed, g, slot, salt, (uint32_t)p);
            fx[p] = sv_aug_uniform_pm1(w.v[0]);
            fy[p] = sv_aug_uniform_pm1(w.v[1]);
        }
        __syncthreads();
        const float *taps = st.f + 1;
        aug_field_pass(fx, ft, H, W, taps, r, true, tid);
        __syncthreads();
        aug_field_pass(ft, fx, H, W, taps, r, false, tid);
        __syncthreads();
        aug_field_pass(fy, ft, H, W, taps, r, true, tid);
        __syncthreads();
        aug_field_pass(ft, fy, H, W, taps, r, false, tid);
        __syncthreads();
        const float alpha = st.f[0];
        for (int p = tid; p < HW; p += 256) {
            const int y = p / W, x = p - y * W;
            const float mx = __fadd_rn((float)x, __fmul_rn(fx[p], alpha)), my = __fadd_rn((float)y, __fmul_rn(fy[p], alpha));
            int sx, sy, a, b;
            sv_remap_split(sv_sat_int((double)__fmul_rn(mx, 32.f)), sv_sat_int((double)__fmul_rn(my, 32.f)), sx, sy, a, b);
            out[p] = (u8)sv_remap_sample(in, H, W, W, sx, sy, a, b, -1);
        }
        break;
    }
    case SV_AUG_NOISE_GAUSS: {
        const double sigma = st.d[0];
        for (int p = tid; p < HW; p += 256) {
            const sv_philox4 w = sv_aug_draw(seed, g, slot, salt, (uint32_t)p);
            out[p] = aug_clip_trunc(__dadd_rn((double)in[p], __dmul_rn(sigma, sv_aug_normal(w.v[0], w.v[1]))));
        }
        break;
    }
    case SV_AUG_NOISE_SP: {
        const double t = st.d[0];
        for (int p = tid; p < HW; p += 256) {
            const sv_philox4 w = sv_aug_draw(seed, g, slot, salt, (uint32_t)p);
            u8 v = in[p];
            if (sv_aug_uniform01(w.v[0]) < t) v = 255;
            if (sv_aug_uniform01(w.v[1]) < t) v = 0;
            out[p] = v;
        }
        break;
    }
    default: wrote = false; break;                         // SV_AUG_NONE and anything unknown: the identity
    }
    return wrote;
}

}  // namespace
