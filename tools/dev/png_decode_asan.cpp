// Host-side check of the PNG decoder under AddressSanitizer + UBSan (host code only; no Python, no GPU):
//   hipcc -O1 -g -std=c++17 -ffp-contract=off -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
//         -I sudoku-vision_amd/csrc tools/dev/png_decode_asan.cpp -o /tmp/png_decode_asan -lpthread && /tmp/png_decode_asan
// 1. sv_png_parse and sv_png_inflate (csrc/host_png.cpp) over valid files -- stored, fixed and dynamic blocks written by the small deflater below,
//    every colour type and depth -- whose inflated bytes must be the filtered bytes they were made from, with the output buffer exactly
//    filtered_bytes long so that one byte too many is a report; then over mutants of them: byte flips, truncation at every length of the small
//    files, and the IDAT payload re-split at every boundary (which must decode as before).  A mutant may be refused or, where the flip hit an
//    ancillary detail, accepted; it may not crash, read or write out of bounds.
// 2. The arithmetic the kernels share with the host (csrc/sv_png_pixel.h): unfilter_byte for filter bytes 0..6 over a grid of (a, b, c) dense at 0, 128 and 255,
//    against a restatement in long arithmetic, and expand_pixel over every format with the row buffer exactly row_bytes long.
// The unfilter's KERNELS are not plain functions of the thread id (they hand values across lanes of a wave), so they are not looped over here; the GPU
// tests check them.
#include "../../sudoku-vision_amd/csrc/host_png.cpp"
#include "../../sudoku-vision_amd/csrc/sv_png_pixel.h"
#include <random>
static thread_local char g_msg[256] = "";
int sv_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char *sv_last_error(void) { return g_msg; }

namespace {

typedef std::vector<uint8_t> Bytes;

struct BitOut {
    Bytes out; uint32_t buf = 0; int cnt = 0;
    void put(uint32_t v, int n) { for (int i = 0; i < n; i++) { buf |= ((v >> i) & 1u) << cnt; if (++cnt == 8) { out.push_back((uint8_t)buf); buf = 0; cnt = 0; } } }
    void code(uint32_t v, int n) { for (int i = n - 1; i >= 0; i--) put((v >> i) & 1u, 1); }
    void flush() { if (cnt) { out.push_back((uint8_t)buf); buf = 0; cnt = 0; } }
};

// canonical codes of a set of lengths
struct Code {
    std::vector<int> len, code;
    explicit Code(const std::vector<int> &l) : len(l), code(l.size(), 0)
    {
        int next = 0;
        for (int n = 1; n < 16; n++, next <<= 1)
            for (size_t s = 0; s < l.size(); s++)
                if (l[s] == n) code[s] = next++;
    }
    void put(BitOut &w, int s) const { w.code((uint32_t)code[(size_t)s], len[(size_t)s]); }
};

std::vector<int> literal_lengths(int mode)
{
    std::vector<int> l(mode == 1 ? 288 : 286);
    for (size_t i = 0; i < l.size(); i++) l[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : (mode == 1 || i < 284) ? 8 : 7;      // 286 codes: two 7-bit ones fill the gap
    return l;
}

// mode 0: stored blocks of at most `piece` bytes; 1: one fixed block, runs as distance-1 matches; 2: a dynamic block with a 7/8/9-bit literal code
// (the fixed code's lengths but for the last two, sent explicitly) and one distance code of one bit
Bytes zlib_stream(const Bytes &raw, int mode, size_t piece)
{
    BitOut w;
    w.put(0x78, 8); w.put(0x9c, 8);
    const Code lit(literal_lengths(mode));
    if (mode == 0) {
        size_t at = 0;
        do {
            const size_t n = std::min(piece, raw.size() - at);
            w.put(at + n == raw.size(), 1); w.put(0, 2); w.flush();
            w.put((uint32_t)n, 16); w.put((uint32_t)n ^ 0xffffu, 16);
            for (size_t i = 0; i < n; i++) w.put(raw[at + i], 8);
            at += n;
        } while (at < raw.size());
    } else {
        w.put(1, 1); w.put(mode, 2);
        if (mode == 2) {
            w.put(288 - 2 - 257, 5); w.put(0, 5); w.put(19 - 4, 4);      // HLIT 286, HDIST 1, all 19 code-length lengths
            static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            for (int s : order) w.put(s == 1 || s == 7 || s == 8 || s == 9 ? 2 : 0, 3);    // four 2-bit codes: 1 -> 00, 7 -> 01, 8 -> 10, 9 -> 11
            for (int i = 0; i < 286; i++) w.code((uint32_t)lit.len[(size_t)i] - 6, 2);
            w.code(0, 2);                                                // the distance code: length 1
        }
        for (size_t i = 0; i < raw.size();) {
            size_t run = 0;
            if (i > 0) while (i + run < raw.size() && raw[i + run] == raw[i - 1] && run < 258) run++;
            if (run >= 3) {
                static const int lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
                static const int lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
                int s = 28;
                while (lbase[s] > (int)run) s--;
                if (s == 28 && run != 258) s = 27;
                if (lbase[s] + (1 << lext[s]) - 1 < (int)run) run = (size_t)(lbase[s] + (1 << lext[s]) - 1);
                lit.put(w, 257 + s);
                w.put((uint32_t)run - (uint32_t)lbase[s], lext[s]);
                if (mode == 1) w.code(0, 5); else w.code(0, 1);         // distance 1
                i += run;
            } else {
                lit.put(w, raw[i++]);
            }
        }
        lit.put(w, 256);
    }
    w.flush();
    uint32_t a = 1, b = 0;
    for (uint8_t v : raw) { a = (a + v) % 65521; b = (b + a) % 65521; }
    for (int k = 3; k >= 0; k--) w.out.push_back((uint8_t)((b << 16 | a) >> (8 * k)));
    return w.out;
}

void put_chunk(Bytes &f, const char *type, const uint8_t *body, size_t n)
{
    uint8_t head[8];
    be32(head, (uint32_t)n); memcpy(head + 4, type, 4);
    f.insert(f.end(), head, head + 8);
    f.insert(f.end(), body, body + n);
    Bytes crc_in(head + 4, head + 8);
    crc_in.insert(crc_in.end(), body, body + n);
    uint8_t crc[4];
    be32(crc, crc32_update(0, crc_in.data(), crc_in.size()));
    f.insert(f.end(), crc, crc + 4);
}

Bytes png_file(int w, int h, int type, int depth, const Bytes &payload, const std::vector<size_t> &cuts)
{
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    Bytes f(sig, sig + 8);
    uint8_t ihdr[13];
    be32(ihdr, (uint32_t)w); be32(ihdr + 4, (uint32_t)h);
    ihdr[8] = (uint8_t)depth; ihdr[9] = (uint8_t)type; ihdr[10] = ihdr[11] = ihdr[12] = 0;
    put_chunk(f, "IHDR", ihdr, 13);
    if (type == 3) { uint8_t pal[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12}; put_chunk(f, "PLTE", pal, 12); }
    uint8_t gama[4] = {0, 0, 0xb1, 0x8f};
    put_chunk(f, "gAMA", gama, 4);
    size_t at = 0;
    for (size_t c : cuts) { put_chunk(f, "IDAT", payload.data() + at, c - at); at = c; }
    put_chunk(f, "IDAT", payload.data() + at, payload.size() - at);
    put_chunk(f, "IEND", nullptr, 0);
    return f;
}

long g_accepted = 0, g_refused = 0;

// parse + inflate with buffers of exactly the sizes the info states; returns whether the file decoded, and its bytes
bool decode(const Bytes &file, Bytes *out)
{
    std::unique_ptr<uint8_t[]> copy(new uint8_t[file.size() ? file.size() : 1]);      // an exact-size heap copy: reading past the file is a report
    if (!file.empty()) memcpy(copy.get(), file.data(), file.size());
    sv_png_info info;
    if (sv_png_parse(copy.get(), file.size(), &info) != SV_OK) { g_refused++; return false; }
    Bytes filtered((size_t)info.filtered_bytes), rows((size_t)info.height);
    if (sv_png_inflate(copy.get(), file.size(), &info, filtered.data(), filtered.size(), rows.data()) != SV_OK) { g_refused++; return false; }
    g_accepted++;
    if (out) *out = filtered;
    return true;
}

int fail(const char *what) { fprintf(stderr, "png_decode_asan: %s (%s)\n", what, g_msg); return 1; }

}  // namespace

int main()
{
    std::mt19937 rng(19);
    static const int formats[15][2] = {{0, 1}, {0, 2}, {0, 4}, {0, 8}, {0, 16}, {2, 8}, {2, 16}, {3, 1}, {3, 2}, {3, 4}, {3, 8}, {4, 8}, {4, 16}, {6, 8}, {6, 16}};
    long files = 0, flips = 0, truncations = 0, resplits = 0;
    for (int fi = 0; fi < 15; fi++)
        for (int shape = 0; shape < 4; shape++)
            for (int mode = 0; mode < 3; mode++) {
                const int type = formats[fi][0], depth = formats[fi][1];
                const int w = shape == 0 ? 1 : shape == 1 ? 7 : shape == 2 ? 33 : 300, h = shape == 0 ? 1 : shape == 1 ? 5 : shape == 2 ? 9 : 260;
                const int ch = png_channels(type);
                const size_t row = ((size_t)w * ch * depth + 7) / 8;
                Bytes raw((1 + row) * (size_t)h);
                for (size_t i = 0; i < raw.size(); i++) raw[i] = (rng() % 4) ? (uint8_t)(i / 5) : (uint8_t)rng();
                for (int r = 0; r < h; r++) raw[(size_t)r * (1 + row)] = (uint8_t)(rng() % 5);
                const Bytes payload = zlib_stream(raw, mode, shape == 3 ? 65535 : 11);
                const Bytes file = png_file(w, h, type, depth, payload, {});
                Bytes got;
                files++;
                if (!decode(file, &got) || got != raw) return fail("a valid file did not inflate to its filtered bytes");
                const bool small = shape < 3;
                // the IDAT payload re-split at every boundary (small files) or at 64 random ones
                for (size_t c = 0; c <= (small ? payload.size() : 64); c++) {
                    const size_t cut = small ? c : rng() % (payload.size() + 1);
                    std::vector<size_t> cuts = {cut};
                    if (c % 3 == 0) cuts.push_back(cut);                 // an empty IDAT too
                    resplits++;
                    if (!decode(png_file(w, h, type, depth, payload, cuts), &got) || got != raw) return fail("a re-split file decoded differently");
                }
                // truncation at every length (small files) or at 64 random lengths
                for (size_t c = 0; c < (small ? file.size() : 64); c++) {
                    const size_t len = small ? c : rng() % file.size();
                    truncations++;
                    if (decode(Bytes(file.begin(), file.begin() + (long)len), nullptr)) return fail("a truncated file was accepted");
                }
                // byte flips: in the IDAT payload with the CRC mended (so the inflater sees them), and anywhere with the CRC left wrong
                const size_t n_flips = small ? 400 : 60;
                for (size_t k = 0; k < n_flips; k++) {
                    Bytes bad = payload;
                    const int hits = 1 + (int)(rng() % 3);
                    for (int j = 0; j < hits; j++) bad[rng() % bad.size()] ^= (uint8_t)(1u << (rng() % 8));
                    flips++;
                    decode(png_file(w, h, type, depth, bad, small ? std::vector<size_t>{bad.size() / 2} : std::vector<size_t>{}), nullptr);
                    Bytes anywhere = file;
                    anywhere[rng() % anywhere.size()] ^= (uint8_t)(1u << (rng() % 8));
                    flips++;
                    decode(anywhere, nullptr);
                }
            }
    // 2. the shared arithmetic
    long bytes_checked = 0, pixels = 0;
    for (unsigned f = 0; f < 7; f++)
        for (unsigned a = 0; a < 256; a += (a < 4 || a > 250 || (a > 124 && a < 132)) ? 1 : 7)
            for (unsigned b = 0; b < 256; b += (b < 4 || b > 250 || (b > 124 && b < 132)) ? 1 : 5)
                for (unsigned c = 0; c < 256; c += (c < 4 || c > 250 || (c > 124 && c < 132)) ? 1 : 3) {
                    const unsigned x = (a * 31 + b * 17 + c * 7 + f) & 255;
                    long pred = 0;
                    if (f == 1) pred = a; else if (f == 2) pred = b; else if (f == 3) pred = ((long)a + b) / 2;
                    else if (f == 4) {
                        const long p = (long)a + b - c, pa = labs(p - a), pb = labs(p - b), pc = labs(p - c);
                        pred = pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
                    }
                    bytes_checked++;
                    if (svpng::unfilter_byte(f, x, a, b, c) != (unsigned)((x + pred) % 256)) return fail("unfilter_byte disagrees with the specification");
                }
    for (int fi = 0; fi < 15; fi++)
        for (int w = 1; w <= 19; w++) {
            const int type = formats[fi][0], depth = formats[fi][1], ch = png_channels(type);
            const size_t row = ((size_t)w * ch * depth + 7) / 8;
            std::unique_ptr<uint8_t[]> line(new uint8_t[row]);
            for (size_t i = 0; i < row; i++) line[i] = (uint8_t)rng();
            uint8_t pal[768];
            for (int i = 0; i < 768; i++) pal[i] = (uint8_t)rng();
            const svpng::Expand e = {type, depth, ch};
            for (int x = 0; x < w; x++) {
                const uint32_t px = svpng::expand_pixel(e, line.get(), x, pal, 200);
                pixels++;
                unsigned s0;
                if (depth >= 8) s0 = line[(size_t)x * ch * (depth / 8)];
                else s0 = (line[(size_t)x * depth / 8] >> (8 - depth - (x * depth) % 8)) & ((1u << depth) - 1);
                uint32_t want;
                if (type == 3) want = s0 >= 200 ? 1u << 24 : (uint32_t)pal[3 * s0 + 2] | (uint32_t)pal[3 * s0 + 1] << 8 | (uint32_t)pal[3 * s0] << 16;
                else if (type == 0 || type == 4) { const unsigned g = depth < 8 ? s0 * (255u / ((1u << depth) - 1)) : s0; want = g * 0x010101u; }
                else { const size_t st = depth / 8; const uint8_t *p = line.get() + (size_t)x * ch * st; want = (uint32_t)p[2 * st] | (uint32_t)p[st] << 8 | (uint32_t)p[0] << 16; }
                if (px != want) return fail("expand_pixel disagrees with the rules");
            }
        }
    printf("png_decode_asan: %ld valid files, %ld re-splits, %ld truncations, %ld byte-flip mutants; %ld decodes accepted, %ld refused; %ld unfilter bytes, %ld pixels: no failure\n",
           files, resplits, truncations, flips, g_accepted, g_refused, bytes_checked, pixels);
    return 0;
}
