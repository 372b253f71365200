// Stand-alone sanitizer check of the host MC-dropout mask generator (csrc/sv_philox.h: sv_mc_masks_fill, what sv_mc_dropout_masks_host
// runs).  Host code only; never loaded into Python and never run on a GPU machine:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/dev/mc_masks_ubsan.cpp -o mc_masks_ubsan && ./mc_masks_ubsan
// Fills exactly-sized heap buffers over the shapes and rates of tests/test_model_v3_mc_ref.py, checks the Random123 known answers, the
// two exact rates and that a cell's bits do not depend on the batch around it.  Exits 0 when clean.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sudoku-vision_amd/csrc/sv_philox.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

int main()
{
    const sv_philox4 a = sv_philox4x32_10(0, 0, 0, 0, 0, 0), b = sv_philox4x32_10(~0u, ~0u, ~0u, ~0u, ~0u, ~0u);
    const sv_philox4 c = sv_philox4x32_10(0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u);
    CHECK(a.v[0] == 0x6627e8d5u && a.v[1] == 0xe169c58du && a.v[2] == 0xbc57ac4cu && a.v[3] == 0x9b00dbd8u);
    CHECK(b.v[0] == 0x408f276du && b.v[1] == 0x41c83b0eu && b.v[2] == 0xa20bc7c6u && b.v[3] == 0x6d5451fdu);
    CHECK(c.v[0] == 0xd16cfe09u && c.v[1] == 0x94fdccebu && c.v[2] == 0x5001e420u && c.v[3] == 0x24126ea1u);
    CHECK(sv_mc_keep_threshold(0.f) == 4294967296ull && sv_mc_keep_threshold(1.f) == 0 && sv_mc_keep_threshold(0.5f) == 2147483648ull);

    const uint64_t seeds[2] = {0x1234567887654321ull, ~0ull}, offsets[2] = {8, ~0ull};
    const int shapes[3][2] = {{1, 1}, {3, 2}, {10, 81}};
    const float rates[4][2] = {{0.f, 0.f}, {0.1f, 0.5f}, {0.5f, 1.f}, {0.1f, 0.1f}};
    for (int k = 0; k < 2; k++)
        for (auto &sh : shapes)
            for (auto &r : rates) {
                const int S = sh[0];
                const long B = sh[1];
                std::vector<uint8_t> k1((size_t)S * B * 32, 7), k3((size_t)S * B * 64, 7), kf((size_t)S * B * 128, 7);
                sv_mc_masks_fill(seeds[k], offsets[k], S, B, r[0], r[1], k1.data(), k3.data(), kf.data());
                long kept = 0;
                for (uint8_t v : k1) { CHECK(v <= 1); kept += v; }
                for (uint8_t v : kf) CHECK(v <= 1 && (r[1] != 1.f || v == 0) && (r[1] != 0.f || v == 1));
                if (r[0] == 0.f) CHECK(kept == (long)k1.size());
                // cell B - 1 of sample S - 1, drawn alone through the generator's own function, is what the batch holds
                for (int g = 0; g < 16; g++) {
                    const sv_philox4 w = sv_mc_draw(seeds[k], offsets[k], (uint32_t)(S - 1), (uint32_t)(B - 1), 1, g);
                    for (int j = 0; j < 4; j++) CHECK(k3[((size_t)(S - 1) * B + (B - 1)) * 64 + 4 * g + j] == ((uint64_t)w.v[j] < sv_mc_keep_threshold(r[0])));
                }
                sv_mc_masks_fill(seeds[k], offsets[k], S, B, r[0], r[1], nullptr, nullptr, nullptr);       // every output may be NULL
            }
    std::printf(fails ? "mc_masks_ubsan: %d checks failed\n" : "mc_masks_ubsan: clean\n", fails);
    return fails != 0;
}
