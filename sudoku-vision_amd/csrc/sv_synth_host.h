// K23 (k23_synth_cells.hip) in plain C++ with nothing of HIP but the SV_HD mark: phase A's pixel, the per-pixel bodies of the new
// phase-B ops with all their clamping and clipping, the program check and the tap helper.  The kernel calls these very functions, and
// tools/dev/synth_program_ubsan.cpp compiles them with a host compiler alone and runs them over malformed records under ASan / UBSan.
// include/sudoku_vision_hip.h states every rule.  Compiled with -ffp-contract=off: every operation below is rounded on its own.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/sudoku_vision_hip.h"
#include "sv_augment_host.h"
#include "sv_philox.h"

SV_HD inline int sv_syn_clampi(long long v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }
SV_HD inline uint8_t sv_syn_clip_trunc(double v) { return (uint8_t)(int)fmin(fmax(v, 0.0), 255.0); }     // NaN -> 0 (fmax drops it)
SV_HD inline int sv_syn_reflect101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}
SV_HD inline float sv_syn_div255(float v)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __fdiv_rn(v, 255.0f);
#else
    return v / 255.0f;
#endif
}

// Phase A: pixel (x, y) of output g's base image; prev is the output's own size*size bytes (SV_SYN_BG_KEEP).  atlas / dims may be NULL when n_slots is 0.
SV_HD inline uint8_t sv_syn_base_pixel(const sv_syn_cell &c, int size, int x, int y, uint64_t seed, uint64_t g, const uint8_t *atlas, const int32_t *dims, int n_slots, const uint8_t *prev)
{
    const int base = sv_syn_clampi(c.bg_value, 0, 255);
    int p = base;
    if (c.bg_kind == SV_SYN_BG_TEXTURED || c.bg_kind == SV_SYN_BG_NOISY) {
        const sv_philox4 w = sv_aug_draw(seed, g, SV_SYN_BG_SLOT, (uint32_t)c.bg_salt, (uint32_t)(y * size + x));
        p = sv_syn_clip_trunc((double)base + c.bg_d[0] * sv_aug_normal(w.v[0], w.v[1]));
        const int stride = c.grain_stride;
        if (c.bg_kind == SV_SYN_BG_TEXTURED && stride >= 2 && stride <= 4 && y % stride == 0) {
            const int k = y / stride;                                                       // < 32: y < 64, stride >= 2
            const int d = (int)((c.grain_d[k >> 4] >> (2 * (k & 15))) & 3u);
            p = p - d > 0 ? p - d : 0;
        }
    } else if (c.bg_kind == SV_SYN_BG_KEEP) {
        p = prev[y * size + x];
    } else if (c.bg_kind == SV_SYN_BG_GRADIENT) {
        if (c.grad_dir == 0 || c.grad_dir == 1) {
            const int i = c.grad_dir == 0 ? x : y;
            const double t = i == size - 1 ? c.bg_d[2] : (double)i * c.bg_d[1] + c.bg_d[0];
            p = sv_syn_clip_trunc((double)base + t);
        } else if (c.grad_dir == 2) {
            const int ctr = size / 2, dx = x - ctr, dy = y - ctr;
            const double t = (sqrt((double)(dx * dx + dy * dy)) / ((double)size / 2.0)) * c.bg_d[0];
            p = sv_syn_clip_trunc((double)base - t);
        }
    }
    const int aw = sv_syn_clampi(c.art_width, 0, 2), ad = sv_syn_clampi(c.art_dark, 0, 255);
    if (((c.art_edges & 1) && y < aw) || ((c.art_edges & 2) && y >= size - aw) || ((c.art_edges & 4) && x < aw) || ((c.art_edges & 8) && x >= size - aw))
        p = p < ad ? p : ad;
    const long long sx0 = c.smudge[0], sy0 = c.smudge[1], side = sv_syn_clampi(c.smudge[2], 0, size);
    if (x >= sx0 && x < sx0 + side && y >= sy0 && y < sy0 + side) {
        const int sd = sv_syn_clampi(c.smudge[3], 0, 255);
        p = p < sd ? p : sd;
    }
    if (c.glyph_slot >= 0 && c.glyph_slot < n_slots) {
        const int gw = sv_syn_clampi(dims[2 * c.glyph_slot], 0, SV_SYN_GLYPH_SIDE), gh = sv_syn_clampi(dims[2 * c.glyph_slot + 1], 0, SV_SYN_GLYPH_SIDE);
        const long long mx = (long long)x - c.glyph_x, my = (long long)y - c.glyph_y;
        int m = 0;
        if (mx >= 0 && mx < gw && my >= 0 && my < gh) m = atlas[((size_t)c.glyph_slot * SV_SYN_GLYPH_SIDE + (size_t)my) * SV_SYN_GLYPH_SIDE + (size_t)mx];
        const int t = sv_syn_clampi(c.glyph_ink, 0, 255) * m + 255 * (255 - m) + 128;
        const int digit = (t + (t >> 8)) >> 8;
        p = (int)sv_syn_div255((float)p * (float)digit);
    }
    return (uint8_t)p;
}

// SV_SYN_GAUSS_BLUR at (x, y): k is 3 or 5 (the caller makes any other k the identity); taps clamped to 0..256 so that the sum fits 31 bits
SV_HD inline uint8_t sv_syn_blur_px(const uint8_t *in, int H, int W, int x, int y, int k, const int32_t *taps)
{
    const int r = k >> 1;
    const unsigned t[3] = {(unsigned)sv_syn_clampi(taps[0], 0, 256), (unsigned)sv_syn_clampi(taps[1], 0, 256), (unsigned)sv_syn_clampi(taps[2], 0, 256)};
    unsigned acc = 0;
    for (int j = -r; j <= r; j++) {
        const uint8_t *row = in + sv_syn_reflect101(y + j, H) * W;
        unsigned h = 0;
        for (int i = -r; i <= r; i++) h += t[i < 0 ? -i : i] * row[sv_syn_reflect101(x + i, W)];
        acc += t[j < 0 ? -j : j] * h;
    }
    acc = (acc + 32768u) >> 16;
    return (uint8_t)(acc > 255u ? 255u : acc);
}

// SV_SYN_ERODE (dilate = false) / SV_SYN_DILATE at (x, y): over (x-1..x, y-1..y), taps outside the image ignored
SV_HD inline uint8_t sv_syn_morph_px(const uint8_t *in, int H, int W, int x, int y, bool dilate)
{
    (void)H;
    int v = in[y * W + x];
    for (int j = -1; j <= 0; j++)
        for (int i = -1; i <= 0; i++) {
            if (x + i < 0 || y + j < 0) continue;
            const int q = in[(y + j) * W + (x + i)];
            v = dilate ? (q > v ? q : v) : (q < v ? q : v);
        }
    return (uint8_t)v;
}

// the Q8.8 taps by distance (sv_synth_gaussian_taps_q8); false for a k or sigma outside the contract
inline bool sv_syn_gaussian_taps_q8(int k, double sigma, int32_t *taps)
{
    if ((k != 3 && k != 5) || !(sigma > 0) || !std::isfinite(sigma)) return false;
    const int r = k / 2;
    double v[3] = {1.0, 0.0, 0.0}, sum = 1.0;
    for (int j = 1; j <= r; j++) {
        v[j] = std::exp(-(double)(j * j) / (2.0 * sigma * sigma));
        sum += 2.0 * v[j];
    }
    taps[1] = (int32_t)std::nearbyint(v[1] / sum * 256.0);
    taps[2] = r == 2 ? (int32_t)std::nearbyint(v[2] / sum * 256.0) : 0;
    taps[0] = 256 - 2 * taps[1] - 2 * taps[2];
    return true;
}

// SV_OK, or SV_ERR_BAD_ARG with the reason in msg
inline int sv_syn_check_program(const sv_syn_cell *cells, const sv_aug_step *steps, const int32_t *n_steps, long n_out, int size, const int32_t *dims, int n_slots,
                                char *msg, size_t cap)
{
#define SV_SYN_REFUSE(...) do { snprintf(msg, cap, __VA_ARGS__); return SV_ERR_BAD_ARG; } while (0)
    if (!cells || !steps || !n_steps || (n_slots > 0 && !dims)) SV_SYN_REFUSE("NULL argument");
    if (n_out < 1 || n_slots < 0 || size < 4 || size > SV_AUG_MAX_SIDE) SV_SYN_REFUSE("bad shape: n_out %ld, n_slots %d, size %d (4..%d)", n_out, n_slots, size, SV_AUG_MAX_SIDE);
    auto finite = [](const double *d, int n) { for (int k = 0; k < n; k++) if (!std::isfinite(d[k])) return false; return true; };
    auto byte = [](int v) { return v >= 0 && v <= 255; };
    for (int s = 0; s < n_slots; s++)
        if (dims[2 * s] < 1 || dims[2 * s + 1] < 1 || dims[2 * s] > SV_SYN_GLYPH_SIDE || dims[2 * s + 1] > SV_SYN_GLYPH_SIDE)
            SV_SYN_REFUSE("atlas slot %d: mask of %d x %d (sides 1..%d)", s, dims[2 * s], dims[2 * s + 1], SV_SYN_GLYPH_SIDE);
    for (long o = 0; o < n_out; o++) {
        const sv_syn_cell &c = cells[o];
        if (c.bg_kind < SV_SYN_BG_PLAIN || c.bg_kind > SV_SYN_BG_KEEP) SV_SYN_REFUSE("output %ld bg_kind: unknown kind %d", o, c.bg_kind);
        if (!byte(c.bg_value)) SV_SYN_REFUSE("output %ld bg_value: %d outside 0..255", o, c.bg_value);
        if (c.bg_kind == SV_SYN_BG_TEXTURED || c.bg_kind == SV_SYN_BG_NOISY) {
            if (!finite(c.bg_d, 1)) SV_SYN_REFUSE("output %ld bg_d: sigma is not finite", o);
        } else if (c.bg_kind == SV_SYN_BG_GRADIENT) {
            if (c.grad_dir < 0 || c.grad_dir > 2) SV_SYN_REFUSE("output %ld grad_dir: unknown direction %d", o, c.grad_dir);
            if (!finite(c.bg_d, c.grad_dir == 2 ? 1 : 3)) SV_SYN_REFUSE("output %ld bg_d: gradient term is not finite", o);
        }
        if (c.grain_stride != 0) {
            if (c.grain_stride < 2 || c.grain_stride > 4) SV_SYN_REFUSE("output %ld grain_stride: %d (0 or 2..4)", o, c.grain_stride);
            for (int k = 0; k * c.grain_stride < size; k++)
                if (((c.grain_d[k >> 4] >> (2 * (k & 15))) & 3u) == 0) SV_SYN_REFUSE("output %ld grain_d: row %d has d 0 (1..3)", o, k * c.grain_stride);
        }
        if (c.art_edges < 0 || c.art_edges > 15) SV_SYN_REFUSE("output %ld art_edges: %d outside 0..15", o, c.art_edges);
        if (c.art_edges && (c.art_width < 1 || c.art_width > 2)) SV_SYN_REFUSE("output %ld art_width: %d (1..2)", o, c.art_width);
        if (c.art_edges && !byte(c.art_dark)) SV_SYN_REFUSE("output %ld art_dark: %d outside 0..255", o, c.art_dark);
        if (c.smudge[2] != 0) {
            const int32_t *m = c.smudge;
            if (m[2] < 0 || m[2] > size || m[0] < 0 || m[1] < 0 || m[0] > size - m[2] || m[1] > size - m[2] || !byte(m[3]))
                SV_SYN_REFUSE("output %ld smudge: x %d y %d side %d darkness %d outside the %d x %d cell", o, m[0], m[1], m[2], m[3], size, size);
        }
        if (c.glyph_slot < -1 || c.glyph_slot >= n_slots) SV_SYN_REFUSE("output %ld glyph_slot: %d outside -1..%d", o, c.glyph_slot, n_slots - 1);
        if (c.glyph_slot >= 0 && !byte(c.glyph_ink)) SV_SYN_REFUSE("output %ld glyph_ink: %d outside 0..255", o, c.glyph_ink);
        if (n_steps[o] < 0 || n_steps[o] > SV_AUG_MAX_STEPS) SV_SYN_REFUSE("output %ld: %d steps (0..%d)", o, n_steps[o], SV_AUG_MAX_STEPS);
        for (int s = 0; s < n_steps[o]; s++) {
            const sv_aug_step &st = steps[o * SV_AUG_MAX_STEPS + s];
            const int32_t *i = st.i;
            switch (st.op) {
            case SV_SYN_AFFINE_CONST:
                if (!finite(st.d, 6)) SV_SYN_REFUSE("output %ld step %d: affine matrix is not finite", o, s);
                if (!byte(i[0])) SV_SYN_REFUSE("output %ld step %d: border value %d outside 0..255", o, s, i[0]);
                break;
            case SV_SYN_PERSPECTIVE_CONST:
                if (!finite(st.d, 9)) SV_SYN_REFUSE("output %ld step %d: perspective matrix is not finite", o, s);
                if (!byte(i[0])) SV_SYN_REFUSE("output %ld step %d: border value %d outside 0..255", o, s, i[0]);
                break;
            case SV_SYN_SCALE_PAD: {
                const bool crop = i[2] != 0;
                if (i[0] < 1 || i[1] < 1 || i[0] > 2 * size || i[1] > 2 * size || (i[2] != 0 && i[2] != 1) || (crop ? (i[0] < size || i[1] < size) : (i[0] > size || i[1] > size)))
                    SV_SYN_REFUSE("output %ld step %d: scale to %d x %d (%s) of a %d x %d image", o, s, i[1], i[0], crop ? "crop" : "pad", size, size);
                if (!byte(i[3])) SV_SYN_REFUSE("output %ld step %d: pad value %d outside 0..255", o, s, i[3]);
                break;
            }
            case SV_SYN_GAUSS_BLUR:
                if (i[0] != 3 && i[0] != 5) SV_SYN_REFUSE("output %ld step %d: blur kernel %d (3 or 5)", o, s, i[0]);
                if (i[1] < 0 || i[2] < 0 || i[3] < 0 || i[1] > 256 || i[2] > 256 || i[3] > 256 || (i[0] == 3 && i[3] != 0) || i[1] + 2 * i[2] + 2 * i[3] != 256)
                    SV_SYN_REFUSE("output %ld step %d: blur taps %d %d %d do not sum to 256", o, s, i[1], i[2], i[3]);
                break;
            case SV_SYN_ERODE: case SV_SYN_DILATE: break;
            default: {
                if (st.op < SV_AUG_NONE || st.op > SV_AUG_NOISE_SP) SV_SYN_REFUSE("output %ld step %d: unknown op %d", o, s, st.op);
                const int32_t one = 1, zero = 0;                                   // a K22 op: K22's own rules, on this one record
                char inner[200];
                if (sv_aug_check_program(&st, &one, &zero, 1, 1, size, size, inner, sizeof inner) != SV_OK) {
                    const char *colon = strchr(inner, ':');                       // "output 0 step 0: reason"
                    SV_SYN_REFUSE("output %ld step %d:%s", o, s, colon ? colon + 1 : inner);
                }
            }
            }
        }
    }
#undef SV_SYN_REFUSE
    return SV_OK;
}
