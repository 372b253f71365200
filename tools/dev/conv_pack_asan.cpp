// Host-side check of csrc/sv_conv_f32.h's packers (sv_fold_bn, sv_pack_conv_image) under AddressSanitizer + UBSan (host code only):
//   hipcc -O1 -g -std=c++17 -ffp-contract=off -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
//         -I sudoku-vision_amd/csrc tools/dev/conv_pack_asan.cpp -o /tmp/conv_pack_asan && /tmp/conv_pack_asan
// For every (cout, cin, ks) K8 and K12 pack through the header, with random weights: every element of the image is looked up from its own
// index (N-tile, channel group, tap, lane) and must be the folded weight of that (oc, ic, tap), or zero in the padding.
#include <cstdio>
#include <random>

#include "sv_conv_f32.h"

int main()
{
    const struct { int cout, cin, ks; bool bn; } shapes[] = {{32, 1, 3, true}, {64, 32, 1, true}, {128, 128, 3, true}, {48, 24, 3, true}, {32, 16, 3, false}};
    std::mt19937 rng(13);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::uniform_real_distribution<float> ud(0.5f, 2.f);
    long checked = 0, bad = 0;
    for (const auto &sh : shapes) {
        const int cout = sh.cout, cin = sh.cin, taps = sh.ks * sh.ks, g4 = (cin + 3) / 4, nts = (cout + 15) / 16;
        std::vector<float> cw((size_t)cout * cin * taps), gamma(cout), beta(cout), mean(cout), var(cout), b(cout);
        std::vector<double> k(cout);
        for (auto &v : cw) v = nd(rng);
        for (int oc = 0; oc < cout; oc++) { gamma[oc] = nd(rng); beta[oc] = nd(rng); mean[oc] = nd(rng); var[oc] = ud(rng); }
        if (sh.bn) sv_fold_bn(gamma.data(), beta.data(), mean.data(), var.data(), cout, k.data(), b.data());
        const std::vector<float> img = sv_pack_conv_image(cw.data(), sh.bn ? k.data() : nullptr, cout, cin, taps);
        if (img.size() != (size_t)nts * g4 * taps * 64) { printf("(%d,%d,%d): size %zu\n", cout, cin, sh.ks, img.size()); bad++; }
        for (size_t e = 0; e < img.size(); e++, checked++) {
            const int lane = e % 64, t = e / 64 % taps, g = e / 64 / taps % g4, nt = e / 64 / taps / g4;
            const int oc = 16 * nt + (lane & 15), ic = 4 * g + (lane >> 4);
            float want = 0.f;
            if (oc < cout && ic < cin) {
                want = cw[((size_t)oc * cin + ic) * taps + t];
                if (sh.bn) want = (float)((double)want * ((double)gamma[oc] / std::sqrt((double)var[oc] + 1e-5)));
            }
            if (img[e] != want && bad++ < 10) printf("(%d,%d,%d) element %zu: %g, want %g\n", cout, cin, sh.ks, e, img[e], want);
        }
        for (int oc = 0; sh.bn && oc < cout; oc++, checked++) {
            const double kk = (double)gamma[oc] / std::sqrt((double)var[oc] + 1e-5);
            if (b[oc] != (float)((double)beta[oc] - (double)mean[oc] * kk) && bad++ < 10) printf("(%d,%d,%d) bias %d\n", cout, cin, sh.ks, oc);
        }
    }
    printf("%ld values checked, %ld wrong\n", checked, bad);
    return bad != 0;
}
