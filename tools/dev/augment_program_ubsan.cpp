// Stand-alone sanitizer check of K22's host side (csrc/sv_augment_host.h: the program check, the rotation, perspective and tap helpers;
// csrc/sv_philox.h: the K22 draws).  Host code only; never loaded into Python and never run on a GPU machine:
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/dev/augment_program_ubsan.cpp -o augment_program_ubsan && ./augment_program_ubsan
// Runs well-formed and malformed programs (every refusal of the check, extreme integers, NaN and infinity in every float slot, random
// bytes as step records) from exactly-sized heap buffers, the helpers at their edges, and the draws over the whole counter layout.
// Exits 0 when clean.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../sudoku-vision_amd/csrc/sv_augment_host.h"
#include "../../sudoku-vision_amd/csrc/sv_philox.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static sv_aug_step step(int op, std::initializer_list<int> i = {}, std::initializer_list<double> d = {})
{
    sv_aug_step s;
    memset(&s, 0, sizeof s);
    s.op = op;
    int k = 0;
    for (int v : i) s.i[k++] = v;
    k = 0;
    for (double v : d) s.d[k++] = v;
    return s;
}

// one output whose program is `chain`, from heap buffers of exactly the needed size
static int check_chain(const std::vector<sv_aug_step> &chain, int H = 28, int W = 28, int n_steps = -1, int src = 0, const char *expect = nullptr)
{
    std::vector<sv_aug_step> steps(SV_AUG_MAX_STEPS);
    memset(steps.data(), 0, steps.size() * sizeof(sv_aug_step));
    for (size_t k = 0; k < chain.size() && k < steps.size(); k++) steps[k] = chain[k];
    std::vector<int32_t> ns(1, n_steps < -1 ? n_steps : n_steps == -1 ? (int)chain.size() : n_steps), si(1, src);
    std::vector<char> msg(256);
    const int rc = sv_aug_check_program(steps.data(), ns.data(), si.data(), 1, 2, H, W, msg.data(), msg.size());
    if (expect && !(rc == SV_ERR_BAD_ARG && strstr(msg.data(), expect))) { std::printf("expected \"%s\", got rc %d \"%s\"\n", expect, rc, rc ? msg.data() : ""); fails++; }
    return rc;
}

int main()
{
    static_assert(sizeof(sv_aug_step) == 96, "sv_aug_step is 96 bytes");
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();

    // well-formed
    float taps[SV_AUG_MAX_RADIUS + 1];
    const int r3 = sv_aug_elastic_radius(3.0);
    CHECK(r3 == 12);
    sv_aug_elastic_taps(3.0, r3, taps);
    double sum = taps[0];
    for (int j = 1; j <= r3; j++) { sum += 2.0 * taps[j]; CHECK(taps[j] < taps[j - 1] && taps[j] > 0); }
    CHECK(std::fabs(sum - 1.0) < 1e-6);
    sv_aug_step el = step(SV_AUG_ELASTIC, {r3, 0, 0, 0, -7});
    el.f[0] = 8.f;
    memcpy(el.f + 1, taps, sizeof(float) * (r3 + 1));
    CHECK(check_chain({step(SV_AUG_AFFINE, {}, {1, 0, 2, 0, 1, -1}), step(SV_AUG_PERSPECTIVE, {}, {1, 0, 0, 0, 1, 0, 0, 0, 1}), step(SV_AUG_BRIGHTNESS, {}, {-300}),
                       step(SV_AUG_CONTRAST, {}, {1.2}), step(SV_AUG_BLUR, {5}), step(SV_AUG_SCALE, {30, 30, 1}), step(SV_AUG_FILL_RECT, {27, 27, 1, 1, 255}), el,
                       step(SV_AUG_NOISE_GAUSS, {}, {7.65}), step(SV_AUG_NOISE_SP, {}, {0.025})}) == SV_OK);
    CHECK(check_chain({}) == SV_OK && check_chain({el}, 13, 17) == SV_OK && check_chain({step(99)}, 28, 28, 0) == SV_OK);

    // malformed
    check_chain({step(11)}, 28, 28, -1, 0, "unknown op 11");
    check_chain({step(imin)}, 28, 28, -1, 0, "unknown op");
    check_chain({}, 28, 28, 11, 0, "11 steps");
    check_chain({}, 28, 28, imin, 0, "steps");
    check_chain({}, 28, 28, imax, 0, "steps");
    check_chain({}, 28, 28, -1, 2, "source index 2");
    check_chain({}, 28, 28, -1, imin, "source index");
    check_chain({}, 3, 28, -1, 0, "bad shape");
    check_chain({}, 28, imax, -1, 0, "bad shape");
    check_chain({step(SV_AUG_AFFINE, {}, {1, 0, inf, 0, 1, 0})}, 28, 28, -1, 0, "affine matrix is not finite");
    check_chain({step(SV_AUG_PERSPECTIVE, {}, {1, 0, 0, 0, 1, 0, 0, 0, nan})}, 28, 28, -1, 0, "perspective matrix is not finite");
    for (int op : {SV_AUG_BRIGHTNESS, SV_AUG_CONTRAST, SV_AUG_NOISE_GAUSS, SV_AUG_NOISE_SP}) check_chain({step(op, {}, {-inf})}, 28, 28, -1, 0, "parameter is not finite");
    for (int k : {0, 2, 7, -3, imax, imin}) check_chain({step(SV_AUG_BLUR, {k})}, 28, 28, -1, 0, "blur kernel");
    for (auto &s : {step(SV_AUG_SCALE, {29, 27, 1}), step(SV_AUG_SCALE, {28, 29, 0}), step(SV_AUG_SCALE, {57, 57, 1}), step(SV_AUG_SCALE, {0, 5, 0}),
                    step(SV_AUG_SCALE, {imax, imax, 1}), step(SV_AUG_SCALE, {imin, imin, 0}), step(SV_AUG_SCALE, {28, 28, 2})})
        check_chain({s}, 28, 28, -1, 0, "scale to");
    for (auto &s : {step(SV_AUG_FILL_RECT, {27, 0, 2, 1, 0}), step(SV_AUG_FILL_RECT, {-1, 0, 1, 1, 0}), step(SV_AUG_FILL_RECT, {0, 0, 1, 1, 256}),
                    step(SV_AUG_FILL_RECT, {imax, imax, imax, imax, 0}), step(SV_AUG_FILL_RECT, {imin, imin, imin, imin, imin}), step(SV_AUG_FILL_RECT, {1, 1, imax, 1, 0}),
                    step(SV_AUG_FILL_RECT, {0, 28, 0, 1, 0})})
        check_chain({s}, 28, 28, -1, 0, "rectangle");
    for (int r : {17, -1, imax, imin, 28}) check_chain({step(SV_AUG_ELASTIC, {r})}, 28, 28, -1, 0, "elastic radius");
    check_chain({el}, 12, 17, -1, 0, "elastic radius 12");
    sv_aug_step bad_tap = el;
    bad_tap.f[4] = std::numeric_limits<float>::quiet_NaN();
    check_chain({bad_tap}, 28, 28, -1, 0, "tap 4 is not finite");
    {
        std::vector<char> msg(8);                              // a message buffer shorter than the message
        int32_t ns = 1, si = 0;
        sv_aug_step s = step(SV_AUG_FILL_RECT, {imax, imax, imax, imax, imax});
        CHECK(sv_aug_check_program(&s, &ns, &si, 1, 1, 28, 28, msg.data(), msg.size()) == SV_ERR_BAD_ARG && strlen(msg.data()) == 7);
        CHECK(sv_aug_check_program(nullptr, &ns, &si, 1, 1, 28, 28, msg.data(), msg.size()) == SV_ERR_BAD_ARG);
        CHECK(sv_aug_check_program(&s, &ns, &si, 0, 1, 28, 28, msg.data(), msg.size()) == SV_ERR_BAD_ARG);
    }
    // random bytes as step records: any answer, no fault
    {
        const long n_out = 64;
        std::vector<sv_aug_step> steps(n_out * SV_AUG_MAX_STEPS);
        std::vector<int32_t> ns(n_out), si(n_out);
        std::vector<char> msg(256);
        uint32_t *words = (uint32_t *)steps.data();
        int refused = 0;
        for (int round = 0; round < 200; round++) {
            for (size_t k = 0; k < steps.size() * sizeof(sv_aug_step) / 16; k++) {
                const sv_philox4 w = sv_philox4x32_10((uint32_t)k, (uint32_t)round, 0, 0, 1, 2);
                memcpy(words + 4 * k, w.v, 16);
            }
            for (long o = 0; o < n_out; o++) {
                ns[o] = (int32_t)(words[o] % 11);
                si[o] = (int32_t)(words[o + 64] % 2);
                for (int s = 0; s < SV_AUG_MAX_STEPS; s++) steps[o * SV_AUG_MAX_STEPS + s].op = (int32_t)(words[o * 7 + s] % 12);   // mostly known ops, garbage arguments
            }
            refused += sv_aug_check_program(steps.data(), ns.data(), si.data(), n_out, 2, 13 + round % 52, 4 + round % 61, msg.data(), msg.size()) != SV_OK;
        }
        CHECK(refused > 150);
    }

    // helpers
    double m[9];
    sv_aug_rotation_matrix(14, 14, 0.0, 1.0, m);
    CHECK(m[0] == 1 && m[1] == 0 && m[2] == 0 && m[3] == 0 && m[4] == 1 && m[5] == 0);
    for (double a : {15.0, -15.0, 90.0, 1e300, -1e300, inf, nan}) sv_aug_rotation_matrix(32, 2, a, 1.0, m);
    const float sq[8] = {0, 0, 28, 0, 28, 28, 0, 28}, moved[8] = {1.5f, -2, 26, 1, 28.5f, 30, 2, 27}, zero[8] = {0};
    CHECK(sv_perspective_transform(sq, sq, m) && std::fabs(m[0] - 1) < 1e-12 && std::fabs(m[4] - 1) < 1e-12 && std::fabs(m[2]) < 1e-12 && m[8] == 1);
    CHECK(sv_perspective_transform(sq, moved, m) && std::isfinite(m[6]) && std::isfinite(m[7]));
    CHECK(!sv_perspective_transform(zero, zero, m));
    const float nanp[8] = {std::numeric_limits<float>::quiet_NaN(), 0, 28, 0, 28, 28, 0, 28};
    CHECK(!sv_perspective_transform(nanp, sq, m));
    CHECK(sv_aug_elastic_radius(0.0) == -1 && sv_aug_elastic_radius(-1.0) == -1 && sv_aug_elastic_radius(nan) == -1 && sv_aug_elastic_radius(inf) == -1 &&
          sv_aug_elastic_radius(1e300) == -1 && sv_aug_elastic_radius(0.25) == 1 && sv_aug_elastic_radius(4.0) == 16 && sv_aug_elastic_radius(1e-300) == 0);
    for (double sigma : {0.25, 1.0, 4.0, 1e-300}) {
        std::vector<float> t(sv_aug_elastic_radius(sigma) + 1);
        sv_aug_elastic_taps(sigma, (int)t.size() - 1, t.data());
        for (float v : t) CHECK(std::isfinite(v) && v >= 0);
    }

    // the draws: the Random123 known answer through the K22 counter layout, the corners of the layout, the conversions' ranges
    const sv_philox4 z = sv_aug_draw(0, 0, 0, 0, 0);
    CHECK(z.v[0] == 0x6627e8d5u && z.v[1] == 0xe169c58du && z.v[2] == 0xbc57ac4cu && z.v[3] == 0x9b00dbd8u);
    const sv_philox4 f = sv_aug_draw(~0ull, (1ull << 56) - 1, 255, ~0u, ~0u);
    CHECK(f.v[0] == 0x408f276du && f.v[1] == 0x41c83b0eu && f.v[2] == 0xa20bc7c6u && f.v[3] == 0x6d5451fdu);
    const sv_philox4 a = sv_aug_draw(5, 7, 1, 9, 3), b = sv_aug_draw(5, 7 + (1ull << 32), 1, 9, 3), c = sv_aug_draw(5, 7, 2, 9, 3);
    CHECK(memcmp(a.v, b.v, 16) != 0 && memcmp(a.v, c.v, 16) != 0);
    CHECK(sv_aug_uniform_pm1(0) == -1.f && sv_aug_uniform_pm1(~0u) == 1.f - 1.1920928955078125e-07f && sv_aug_uniform01(0) == 0.0 && sv_aug_uniform01(~0u) < 1.0);
    CHECK(std::isfinite(sv_aug_normal(0, 0)) && std::isfinite(sv_aug_normal(~0u, ~0u)) && sv_aug_normal(~0u, 0) == 0.0 && sv_aug_normal(0, 0) > 6.6);
    double s1 = 0, s2 = 0;
    const int N = 200000;
    for (int p = 0; p < N; p++) {
        const sv_philox4 w = sv_aug_draw(42, 1, 0, 0, (uint32_t)p);
        const double v = sv_aug_normal(w.v[0], w.v[1]);
        s1 += v;
        s2 += v * v;
    }
    const double mean = s1 / N, sd = std::sqrt(s2 / N - mean * mean);
    CHECK(std::fabs(mean) < 5 / std::sqrt((double)N) && std::fabs(sd - 1) < 5 / std::sqrt(2.0 * N));

    std::printf(fails ? "%d checks FAILED\n" : "augment_program_ubsan: clean\n", fails);
    return fails ? 1 : 0;
}
