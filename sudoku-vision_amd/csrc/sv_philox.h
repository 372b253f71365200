// The MC-dropout mask generator of sv_cnn3_forward_mc_f32 (k8_cnn_v3.hip) and sv_mc_dropout_masks_host (sv_api.cpp): Philox4x32-10
// (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) in plain C++, the same text for the device and the host.
//
// A keep bit is a pure function of (seed, offset, sample s, cell b, site, channel) -- not of the batch size, the sample count or the
// chunking (include/sudoku_vision_hip.h states the layout):
//     key     = (seed & 0xffffffff, seed >> 32)
//     counter = (b, s, site * 64 + channel / 4 + (bits 32..55 of offset << 8), offset & 0xffffffff)
//     the four output words serve channels 4g .. 4g + 3;  site 0 = layer1's output (32 channels), 1 = layer3's (64), 2 = the features (128)
//     keep    = (uint64)word < llrint((1 - (double)p) * 2^32)          exact at p = 0 (always) and p = 1 (never)
// Needs nothing of HIP: tools/dev/mc_masks_ubsan.cpp compiles it with a host compiler alone.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define SV_HD __host__ __device__
#else
#define SV_HD
#endif

constexpr int SV_MC_SITES = 3;
constexpr int SV_MC_MASK = 32 + 64 + 128;        // keep bytes of one (sample, cell): the three sites one after the other
SV_HD inline int sv_mc_channels(int site) { return 32 << site; }
SV_HD inline int sv_mc_site_offset(int site) { return site == 0 ? 0 : site == 1 ? 32 : 96; }

struct sv_philox4 { uint32_t v[4]; };

SV_HD inline sv_philox4 sv_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return sv_philox4{{c0, c1, c2, c3}};
}

// the four words of channels 4g .. 4g + 3 of `site` for sample s of cell b
SV_HD inline sv_philox4 sv_mc_draw(uint64_t seed, uint64_t offset, uint32_t s, uint32_t b, int site, int g)
{
    const uint32_t c2 = (uint32_t)(site * 64 + g) | ((uint32_t)(offset >> 32) << 8);
    return sv_philox4x32_10(b, s, c2, (uint32_t)offset, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// ---- K22 (k22_augment.hip, sv_augment_field_host): the random block of pixel `pixel` = y*W + x of output g's step slot.
//     key     = (seed & 0xffffffff, seed >> 32)
//     counter = (pixel, g & 0xffffffff, (g >> 32) << 8 | slot, salt)          g < 2^56, slot < 256
// Words 0 and 1 serve the step: the x and y field of the elastic step, (w0, w1) of the Gaussian noise, (salt, pepper) of the other.
SV_HD inline sv_philox4 sv_aug_draw(uint64_t seed, uint64_t g, int slot, uint32_t salt, uint32_t pixel)
{
    return sv_philox4x32_10(pixel, (uint32_t)g, ((uint32_t)(g >> 32) << 8) | (uint32_t)(slot & 255), salt, (uint32_t)seed, (uint32_t)(seed >> 32));
}
// (word >> 8) * 2^-23 - 1 in [-1, 1): every step is exact in float32
SV_HD inline float sv_aug_uniform_pm1(uint32_t w) { return (float)(w >> 8) * 1.1920928955078125e-07f - 1.0f; }
// word * 2^-32 in [0, 1), exact in double
SV_HD inline double sv_aug_uniform01(uint32_t w) { return (double)w * 2.3283064365386963e-10; }
// Box-Muller: u1 = (w0 + 1) * 2^-32 in (0, 1], u2 = w1 * 2^-32; sqrt(-2 ln u1) * cos(2 pi u2), every operation a double rounding
SV_HD inline double sv_aug_normal(uint32_t w0, uint32_t w1)
{
    const double u1 = ((double)w0 + 1.0) * 2.3283064365386963e-10, u2 = sv_aug_uniform01(w1);
    const double r = sqrt(-2.0 * log(u1));
    return r * cos(6.283185307179586 * u2);
}

// a word keeps its channel iff it is below this; 2^32 at p = 0, 0 at p = 1
inline uint64_t sv_mc_keep_threshold(float p) { return (uint64_t)std::llrint((1.0 - (double)p) * 4294967296.0); }

// keep1 u8 [S][B][32], keep3 [S][B][64], keepf [S][B][128] (each may be NULL): 1 = keep.  The host side of k_mc_masks.
inline void sv_mc_masks_fill(uint64_t seed, uint64_t offset, int S, long B, float p_spatial, float p_fc, uint8_t *keep1, uint8_t *keep3, uint8_t *keepf)
{
    uint8_t *const out[SV_MC_SITES] = {keep1, keep3, keepf};
    for (int site = 0; site < SV_MC_SITES; site++) {
        if (!out[site]) continue;
        const uint64_t thr = sv_mc_keep_threshold(site == 2 ? p_fc : p_spatial);
        const int C = sv_mc_channels(site);
        for (int s = 0; s < S; s++)
            for (long b = 0; b < B; b++)
                for (int g = 0; g < C / 4; g++) {
                    const sv_philox4 w = sv_mc_draw(seed, offset, (uint32_t)s, (uint32_t)b, site, g);
                    for (int r = 0; r < 4; r++) out[site][((long)s * B + b) * C + 4 * g + r] = (uint64_t)w.v[r] < thr;
                }
    }
}
