// Stand-alone sanitizer check of K24's record rules (csrc/sv_dataset_rec.h: svds::refuse, what the kernel applies to every record and
// sv_dataset_check_records reports).  Host code only; never loaded into Python and never run on a GPU machine:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/dev/dataset_records_asan.cpp -o dataset_records_asan && ./dataset_records_asan
// For valid records, each malformed kind, every value of every one-byte field and two million records of random bytes, it walks the accesses
// the kernel makes for an ACCEPTED record -- every filtered byte, every sample byte of every pixel (svpng::expand_pixel's reads), the palette
// slot -- against heap buffers of exactly filtered_size and n_palettes * 1024 bytes, so that an acceptance that could read outside them is an
// AddressSanitizer report.  Exits 0 when clean.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sudoku-vision_amd/csrc/sv_dataset_rec.h"
#include "../../sudoku-vision_amd/csrc/sv_png_pixel.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

// what the kernel touches for an accepted record; returns a checksum so that nothing is optimised away
static unsigned walk(const sv_dataset_record &r, const std::vector<uint8_t> &filtered, const std::vector<uint8_t> &palettes, int n_palettes, bool *accepted)
{
    svds::Geom g;
    const char *why = svds::refuse(r, filtered.size(), n_palettes, g);
    *accepted = why == nullptr;
    if (why) return 0;
    CHECK(g.W >= 1 && g.W <= SV_CELLS_MAX_SIDE && g.H >= 1 && g.H <= SV_CELLS_MAX_SIDE && g.row_bytes >= 1 && g.row_bytes <= SV_CELLS_MAX_ROW_BYTES);
    CHECK(g.bpp >= 1 && g.bpp <= 8 && g.row_bytes % g.bpp == 0);
    unsigned sum = 0;
    const uint8_t *src = filtered.data() + g.offset;
    std::vector<uint8_t> raw((size_t)g.H * g.row_bytes);                      // the LDS rows, exactly sized
    for (int i = 0; i < g.H * (1 + g.row_bytes); i++) {
        const int row = i / (1 + g.row_bytes), x = i - row * (1 + g.row_bytes);
        if (x) raw[(size_t)row * g.row_bytes + x - 1] = src[i];
        else sum += svpng::unfilter_byte(src[i], 1, 2, 3, 4);
    }
    const uint8_t *pal = g.color_type == 3 ? palettes.data() + (size_t)r.palette * SV_PNG_PALETTE_STRIDE : nullptr;
    unsigned pal_n = 0;
    if (pal) { uint32_t k; memcpy(&k, pal + 768, 4); pal_n = k < 256u ? k : 256u; }
    const svpng::Expand e = {g.color_type, g.bit_depth, g.channels};
    for (int y = 0; y < g.H; y++)
        for (int x = 0; x < g.W; x++) sum += svpng::expand_pixel(e, raw.data() + (size_t)y * g.row_bytes, x, pal, pal_n);
    return sum;
}

int main()
{
    unsigned sum = 0;
    bool ok;
    const int types[5] = {0, 2, 3, 4, 6}, depths[5] = {1, 2, 4, 8, 16};
    // every pair of the specification at the extreme sides, in a buffer that fits exactly
    for (int t : types)
        for (int d : depths) {
            const int ch = svds::channels_of(t, d);
            for (int w : {1, 2, 9, 28, 63, 64})
                for (int h : {1, 28, 64}) {
                    sv_dataset_record r = {0, (uint16_t)w, (uint16_t)h, (uint8_t)t, (uint8_t)d, (uint16_t)(t == 3 ? 1 : SV_CELLS_NO_PALETTE)};
                    const size_t rb = ((size_t)w * ch * d + 7) / 8, need = (size_t)h * (1 + rb);
                    std::vector<uint8_t> filtered(ch ? need + 5 : 16), palettes(2 * SV_PNG_PALETTE_STRIDE);
                    for (auto &b : filtered) b = (uint8_t)rnd();
                    for (auto &b : palettes) b = (uint8_t)rnd();
                    r.offset = ch ? 5 : 0;
                    sum += walk(r, filtered, palettes, 2, &ok);
                    CHECK(ok == (ch != 0));
                    if (!ch) continue;
                    r.offset = 6;                                        // one byte short
                    sum += walk(r, filtered, palettes, 2, &ok);
                    CHECK(!ok);
                    r.offset = ~0ull;                                    // the sum offset + bytes would wrap
                    sum += walk(r, filtered, palettes, 2, &ok);
                    CHECK(!ok);
                    r.offset = 5;
                    r.palette = 2;                                       // at n_palettes: refused whatever the colour type
                    sum += walk(r, filtered, palettes, 2, &ok);
                    CHECK(!ok);
                    r.palette = SV_CELLS_NO_PALETTE;
                    sum += walk(r, filtered, palettes, 2, &ok);
                    CHECK(ok == (t != 3));
                    r.palette = 0; r.width = 0;
                    sum += walk(r, filtered, palettes, 2, &ok);
                    CHECK(!ok);
                    r.width = (uint16_t)w; r.height = 65;
                    sum += walk(r, filtered, palettes, 2, &ok);
                    CHECK(!ok);
                }
        }
    // every value of the two one-byte fields
    {
        std::vector<uint8_t> filtered(64 * 513), palettes(SV_PNG_PALETTE_STRIDE);
        int accepted = 0;
        for (int t = 0; t < 256; t++)
            for (int d = 0; d < 256; d++) {
                sv_dataset_record r = {0, 64, 64, (uint8_t)t, (uint8_t)d, 0};
                sum += walk(r, filtered, palettes, 1, &ok);
                accepted += ok;
            }
        CHECK(accepted == 15);                                           // the pairs of the specification
    }
    // random bytes as records, against small buffers
    {
        std::vector<uint8_t> filtered(3000), palettes(3 * SV_PNG_PALETTE_STRIDE);
        for (auto &b : filtered) b = (uint8_t)rnd();
        for (auto &b : palettes) b = (uint8_t)rnd();
        long accepted = 0;
        for (long i = 0; i < 2000000; i++) {
            uint64_t w[2] = {rnd(), rnd()};
            if (i & 1) w[0] %= 4000;                                     // offsets near the buffer
            if (i & 2) w[1] &= 0x00031f07007f007full;                    // sides, types, depths and palettes that are often valid
            sv_dataset_record r;
            memcpy(&r, w, sizeof r);
            sum += walk(r, filtered, palettes, 3, &ok);
            accepted += ok;
        }
        std::printf("random records: %ld of 2000000 accepted\n", accepted);
        CHECK(accepted > 0);
    }
    static_assert(sizeof(sv_dataset_record) == 16, "the record is 16 bytes");
    std::printf("checksum %u, %d failures\n", sum, fails);
    return fails ? 1 : 0;
}
