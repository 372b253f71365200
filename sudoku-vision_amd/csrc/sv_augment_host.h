// Host side of K22 (k22_augment.hip): the program check and the helpers that turn the reference's arguments into step records, in
// plain C++ with nothing of HIP, so that sv_api.cpp exports them and tools/dev/augment_program_ubsan.cpp compiles them with a host
// compiler alone.  include/sudoku_vision_hip.h states every rule checked here.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>

#include "../../include/sudoku_vision_hip.h"

// cv2.getPerspectiveTransform: 8x8 LU with partial pivoting in double, OpenCV's elimination order
inline bool sv_perspective_transform(const float *src, const float *dst, double *M)
{
    double a[8][9];  // augmented [A | b]
    for (int i = 0; i < 4; i++) {
        const double sx = src[2 * i], sy = src[2 * i + 1], dx = dst[2 * i], dy = dst[2 * i + 1];
        const double r0[9] = {sx, sy, 1, 0, 0, 0, -sx * dx, -sy * dx, dx};
        const double r1[9] = {0, 0, 0, sx, sy, 1, -sx * dy, -sy * dy, dy};
        memcpy(a[i], r0, sizeof r0);
        memcpy(a[i + 4], r1, sizeof r1);
    }
    for (int i = 0; i < 8; i++) {
        int piv = i;
        for (int j = i + 1; j < 8; j++)
            if (std::fabs(a[j][i]) > std::fabs(a[piv][i])) piv = j;
        if (!(std::fabs(a[piv][i]) >= 2.220446049250313e-16 * 100)) return false;  // also rejects NaN
        if (piv != i)
            for (int j = i; j < 9; j++) std::swap(a[i][j], a[piv][j]);
        const double d = -1 / a[i][i];
        for (int j = i + 1; j < 8; j++) {
            const double alpha = a[j][i] * d;
            for (int k = i + 1; k < 9; k++) a[j][k] += alpha * a[i][k];
        }
    }
    for (int i = 7; i >= 0; i--) {
        double s = a[i][8];
        for (int k = i + 1; k < 8; k++) s -= a[i][k] * a[k][8];
        a[i][8] = s / a[i][i];
    }
    for (int i = 0; i < 8; i++) M[i] = a[i][8];
    M[8] = 1.0;
    return true;
}

// cv2.getRotationMatrix2D
inline void sv_aug_rotation_matrix(double cx, double cy, double angle_deg, double scale, double *m)
{
    const double a = angle_deg * (3.141592653589793 / 180);
    const double alpha = std::cos(a) * scale, beta = std::sin(a) * scale;
    m[0] = alpha;
    m[1] = beta;
    m[2] = (1 - alpha) * cx - beta * cy;
    m[3] = -beta;
    m[4] = alpha;
    m[5] = beta * cx + (1 - alpha) * cy;
}

// radius of cv2.GaussianBlur((0,0), sigma) on float32: ksize = round(8*sigma + 1) | 1 (round half to even, cvRound); -1 for a sigma
// that is not positive and finite or whose kernel has no int
inline int sv_aug_elastic_radius(double sigma)
{
    if (!(sigma > 0) || !std::isfinite(sigma) || sigma > 1e6) return -1;
    return ((int)std::nearbyint(sigma * 8 + 1) | 1) / 2;
}

// taps[j], j = 0..r: the tap at distance j (sv_augment_elastic_taps)
inline void sv_aug_elastic_taps(double sigma, int r, float *taps)
{
    const double scale2x = -0.125 / (sigma * sigma);
    double sum = 0.0;
    for (int j = r; j >= 1; j--) sum += std::exp((double)(4 * j * j) * scale2x);
    sum *= 2.0;
    sum += 1.0;
    const double inv = 1.0 / sum;
    for (int j = 1; j <= r; j++) taps[j] = (float)(std::exp((double)(4 * j * j) * scale2x) * inv);
    taps[0] = (float)inv;
}

// SV_OK, or SV_ERR_BAD_ARG with the reason in msg
inline int sv_aug_check_program(const sv_aug_step *steps, const int32_t *n_steps, const int32_t *src_index, long n_out, int n_src, int H, int W, char *msg, size_t cap)
{
#define SV_AUG_REFUSE(...) do { snprintf(msg, cap, __VA_ARGS__); return SV_ERR_BAD_ARG; } while (0)
    if (!steps || !n_steps || !src_index) SV_AUG_REFUSE("NULL argument");
    if (n_out < 1 || n_src < 1 || H < 4 || W < 4 || H > SV_AUG_MAX_SIDE || W > SV_AUG_MAX_SIDE)
        SV_AUG_REFUSE("bad shape: n_out %ld, n_src %d, %d x %d (sides 4..%d)", n_out, n_src, H, W, SV_AUG_MAX_SIDE);
    auto finite = [](const double *d, int n) { for (int k = 0; k < n; k++) if (!std::isfinite(d[k])) return false; return true; };
    for (long o = 0; o < n_out; o++) {
        if (n_steps[o] < 0 || n_steps[o] > SV_AUG_MAX_STEPS) SV_AUG_REFUSE("output %ld: %d steps (0..%d)", o, n_steps[o], SV_AUG_MAX_STEPS);
        if (src_index[o] < 0 || src_index[o] >= n_src) SV_AUG_REFUSE("output %ld: source index %d outside 0..%d", o, src_index[o], n_src - 1);
        for (int s = 0; s < n_steps[o]; s++) {
            const sv_aug_step &st = steps[o * SV_AUG_MAX_STEPS + s];
            const int32_t *i = st.i;
            switch (st.op) {
            case SV_AUG_NONE: break;
            case SV_AUG_AFFINE:
                if (!finite(st.d, 6)) SV_AUG_REFUSE("output %ld step %d: affine matrix is not finite", o, s);
                break;
            case SV_AUG_PERSPECTIVE:
                if (!finite(st.d, 9)) SV_AUG_REFUSE("output %ld step %d: perspective matrix is not finite", o, s);
                break;
            case SV_AUG_BRIGHTNESS: case SV_AUG_CONTRAST: case SV_AUG_NOISE_GAUSS: case SV_AUG_NOISE_SP:
                if (!finite(st.d, 1)) SV_AUG_REFUSE("output %ld step %d: parameter is not finite", o, s);
                break;
            case SV_AUG_BLUR:
                if (i[0] != 1 && i[0] != 3 && i[0] != 5) SV_AUG_REFUSE("output %ld step %d: blur kernel %d (1, 3 or 5)", o, s, i[0]);
                break;
            case SV_AUG_SCALE: {
                const bool crop = i[2] != 0;
                if (i[0] < 1 || i[1] < 1 || i[0] > 2 * W || i[1] > 2 * H || (i[2] != 0 && i[2] != 1) || (crop ? (i[0] < W || i[1] < H) : (i[0] > W || i[1] > H)))
                    SV_AUG_REFUSE("output %ld step %d: scale to %d x %d (%s) of a %d x %d image", o, s, i[1], i[0], crop ? "crop" : "pad", H, W);
                break;
            }
            case SV_AUG_FILL_RECT:
                if (i[0] < 0 || i[1] < 0 || i[2] < 0 || i[3] < 0 || i[2] > W || i[3] > H || i[0] > W - i[2] || i[1] > H - i[3] || i[4] < 0 || i[4] > 255)
                    SV_AUG_REFUSE("output %ld step %d: rectangle x %d y %d w %d h %d value %d outside the %d x %d image", o, s, i[0], i[1], i[2], i[3], i[4], H, W);
                break;
            case SV_AUG_ELASTIC: {
                if (i[0] < 0 || i[0] > SV_AUG_MAX_RADIUS || i[0] >= (H < W ? H : W))
                    SV_AUG_REFUSE("output %ld step %d: elastic radius %d (at most %d and below min(H, W) = %d)", o, s, i[0], SV_AUG_MAX_RADIUS, H < W ? H : W);
                for (int k = 0; k <= 1 + i[0]; k++)
                    if (!std::isfinite(st.f[k])) SV_AUG_REFUSE("output %ld step %d: elastic alpha or tap %d is not finite", o, s, k);
                break;
            }
            default: SV_AUG_REFUSE("output %ld step %d: unknown op %d", o, s, st.op);
            }
        }
    }
#undef SV_AUG_REFUSE
    return SV_OK;
}
