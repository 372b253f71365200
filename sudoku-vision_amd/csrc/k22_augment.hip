// K22 -- tools/augment_data.py's ten augmentations on MI355X: one launch, one 256-thread workgroup per output image.
//
//   k_augment: the workgroup loads its source image (u8, at most 64 x 64) into an LDS plane, runs the output's program -- up to
//   SV_AUG_MAX_STEPS step records read from device memory -- ping-ponging between two LDS planes, and stores the result once.
//   Between steps the image is u8, as each of the reference's functions returns u8.  Nothing but the first load, the step records
//   and the last store touches HBM.  include/sudoku_vision_hip.h states the arithmetic of every step; the file is compiled with
//   -ffp-contract=off, so every float and double operation below is rounded on its own.
//
//   LDS (dynamic, sized by the image): two u8 planes of H*W bytes (rounded up to 16) and three f32 planes of H*W floats for the
//   elastic step (the two displacement fields and the row pass's temporary): 2*784 + 3*3136 = 10,992 bytes at 28 x 28 (14
//   workgroups fit the 160 KiB of a CU; the 32-wave cap allows 8), 57,344 bytes at 64 x 64 (2 workgroups per CU) -- below the
//   64 KiB a workgroup gets without opting in to more.
//
//   An unknown op is the identity, the step count and the source index are clamped, a rectangle is clipped, a radius or a blur
//   size outside the contract makes its step the identity, and every tap is clamped into the plane: no program can make the kernel
//   touch memory outside its buffers.  sv_augment_check_program (sv_augment_host.h) is what reports a malformed program.
#include "sv_device.h"
#include "sv_internal.h"
#include "sv_philox.h"

namespace {

struct AugShared {
    sv_aug_step st;
    double M[9];
    unsigned sum;
};

// cv2's saturate_cast<int>(double): round half to even, saturating
__device__ __forceinline__ int aug_sat_int(double v) { return __double2int_rn(fmax(-2147483648.0, fmin(2147483647.0, v))); }

// the bilinear sample of cv2's remap at cell (sx, sy), fractions (a, b) / 32, BORDER_REPLICATE: each tap's coordinates clamped
__device__ __forceinline__ u8 aug_sample(const u8 *in, int H, int W, int sx, int sy, int a, int b)
{
    const int w00 = (32 - a) * (32 - b) * 32, w01 = a * (32 - b) * 32, w10 = (32 - a) * b * 32, w11 = a * b * 32;
    const int x0 = sv_clamp(sx, 0, W - 1), x1 = sv_clamp(sx + 1, 0, W - 1), y0 = sv_clamp(sy, 0, H - 1), y1 = sv_clamp(sy + 1, 0, H - 1);
    return (u8)((in[y0 * W + x0] * w00 + in[y0 * W + x1] * w01 + in[y1 * W + x0] * w10 + in[y1 * W + x1] * w11 + 16384) >> 15);
}

__device__ __forceinline__ u8 aug_clip_trunc(double v) { return (u8)(int)fmin(fmax(v, 0.0), 255.0); }

// one pixel of cv2.resize(in, (nw, nh)) at (x, y) of the scaled image: sv_resize_linear_u8's arithmetic
__device__ __forceinline__ int aug_resize_px(const u8 *in, int H, int W, int nh, int nw, int x, int y)
{
    int xo, a0, a1, yo, b0, b1;
    sv_resize_axis(W, nw, x, xo, a0, a1);
    sv_resize_axis(H, nh, y, yo, b0, b1);
    if (xo < 0) { xo = 0; a0 = 2048; a1 = 0; }
    if (xo >= W - 1) { xo = W - 1; a0 = 2048; a1 = 0; }
    const int x1 = xo + 1 < W ? xo + 1 : xo;
    const int y0 = sv_clamp(yo, 0, H - 1), y1 = sv_clamp(yo + 1, 0, H - 1);
    const int t0 = in[y0 * W + xo] * a0 + in[y0 * W + x1] * a1;
    const int t1 = in[y1 * W + xo] * a0 + in[y1 * W + x1] * a1;
    return (((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2;
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

__global__ __launch_bounds__(256) void k_augment(const u8 *__restrict__ src, int n_src, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride,
                                                 const sv_aug_step *__restrict__ steps, const int32_t *__restrict__ n_steps, const int32_t *__restrict__ src_index,
                                                 uint64_t seed, uint64_t index_base, u8 *__restrict__ dst, int plane_bytes)
{
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ AugShared sh;
    const int tid = threadIdx.x, HW = H * W;
    const size_t o = blockIdx.x;
    u8 *plane[2] = {lds, lds + plane_bytes};
    float *fx = (float *)(lds + 2 * plane_bytes), *fy = fx + HW, *ft = fy + HW;

    const u8 *img = src + (ptrdiff_t)sv_clamp(src_index[o], 0, n_src - 1) * img_stride;
    for (int p = tid; p < HW; p += 256) {
        const int y = p / W, x = p - y * W;
        plane[0][p] = img[(ptrdiff_t)y * pitch + x];
    }
    const int ns = sv_clamp(n_steps[o], 0, SV_AUG_MAX_STEPS);
    const uint64_t g = index_base + o;
    int cur = 0;
    for (int slot = 0; slot < ns; slot++) {
        __syncthreads();                                       // the previous step's plane is complete; sh is free
        if (tid < (int)(sizeof(sv_aug_step) / 4)) ((uint32_t *)&sh.st)[tid] = ((const uint32_t *)(steps + o * SV_AUG_MAX_STEPS + slot))[tid];
        if (tid == 32) sh.sum = 0;
        __syncthreads();
        const sv_aug_step &st = sh.st;
        const u8 *in = plane[cur];
        u8 *out = plane[cur ^ 1];
        const uint32_t salt = (uint32_t)st.i[4];
        bool wrote = true;
        switch (st.op) {
        case SV_AUG_AFFINE: {
            if (tid == 0) {
                // cv2.warpAffine without WARP_INVERSE_MAP: invert the forward matrix, this sequence of double operations
                const double *m = st.d;
                double D = __dsub_rn(__dmul_rn(m[0], m[4]), __dmul_rn(m[1], m[3]));
                D = D != 0.0 ? __ddiv_rn(1.0, D) : 0.0;
                const double A11 = __dmul_rn(m[4], D), A22 = __dmul_rn(m[0], D);
                const double m1 = __dmul_rn(m[1], -D), m3 = __dmul_rn(m[3], -D);
                sh.M[0] = A11; sh.M[1] = m1; sh.M[3] = m3; sh.M[4] = A22;
                sh.M[2] = __dsub_rn(__dmul_rn(-A11, m[2]), __dmul_rn(m1, m[5]));
                sh.M[5] = __dsub_rn(__dmul_rn(-m3, m[2]), __dmul_rn(A22, m[5]));
            }
            __syncthreads();
            const double *M = sh.M;
            for (int p = tid; p < HW; p += 256) {
                const int y = p / W, x = p - y * W;
                const double fxd = (double)x, fyd = (double)y;
                const int adelta = aug_sat_int(__dmul_rn(__dmul_rn(M[0], fxd), 1024.0)), bdelta = aug_sat_int(__dmul_rn(__dmul_rn(M[3], fxd), 1024.0));
                const int X0 = (int)((unsigned)aug_sat_int(__dmul_rn(__dadd_rn(__dmul_rn(M[1], fyd), M[2]), 1024.0)) + 16u);
                const int Y0 = (int)((unsigned)aug_sat_int(__dmul_rn(__dadd_rn(__dmul_rn(M[4], fyd), M[5]), 1024.0)) + 16u);
                const int X = (int)((unsigned)X0 + (unsigned)adelta) >> 5, Y = (int)((unsigned)Y0 + (unsigned)bdelta) >> 5;
                out[p] = aug_sample(in, H, W, sv_clamp(X >> 5, -32768, 32767), sv_clamp(Y >> 5, -32768, 32767), X & 31, Y & 31);
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
                out[p] = aug_sample(in, H, W, sx, sy, a, b);
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
                out[p] = ((unsigned)x < (unsigned)nw && (unsigned)y < (unsigned)nh) ? (u8)aug_resize_px(in, H, W, nh, nw, x, y) : (u8)128;
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
                const int X = aug_sat_int((double)__fmul_rn(mx, 32.f)), Y = aug_sat_int((double)__fmul_rn(my, 32.f));
                out[p] = aug_sample(in, H, W, sv_clamp(X >> 5, -32768, 32767), sv_clamp(Y >> 5, -32768, 32767), X & 31, Y & 31);
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
        if (wrote) cur ^= 1;                                   // uniform: st is the same for every thread
    }
    __syncthreads();
    u8 *d = dst + o * (size_t)HW;
    for (int p = tid; p < HW; p += 256) d[p] = plane[cur][p];
}

}  // namespace

int svk_augment(sv_ctx *ctx, const u8 *src, int n_src, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const sv_aug_step *steps, const int32_t *n_steps,
                const int32_t *src_index, long n_out, uint64_t seed, long index_base, u8 *dst, hipStream_t s)
{
    (void)ctx;
    const int plane_bytes = (H * W + 15) & ~15;
    const size_t lds = 2 * (size_t)plane_bytes + 3 * sizeof(float) * (size_t)(H * W);
    hipLaunchKernelGGL(k_augment, dim3((unsigned)n_out), dim3(256), lds, s, src, n_src, H, W, pitch, img_stride, steps, n_steps, src_index, seed, (uint64_t)index_base,
                       dst, plane_bytes);
    SV_LAUNCH_CHECK("k_augment");
    return SV_OK;
}
