// Host-side check of the PNG encoder under AddressSanitizer + UBSan (host code only):
//   hipcc -O1 -g -std=c++17 -ffp-contract=off -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
//         -I sudoku-vision_amd/csrc tools/dev/png_encode_asan.cpp -o /tmp/png_encode_asan -lpthread && /tmp/png_encode_asan
// 1. The host half (csrc/host_png.cpp: sv_png_encode_plan, sv_png_assemble, _batch) is fed random band lengths: the file has exactly the size
//    reported, is refused when the buffer is a byte short or a band is longer than its bound, and the batch writes the same bytes on 1 and 4 threads.
// 2. The band algorithm of the device half (csrc/sv_png_band.h) is run phase by phase as plain loops over the 256 thread ids (forwards for even bands,
//    backwards for odd ones: a phase must not depend on the order of its threads), every array access under the sanitizer, and the assembled file's
//    IDAT is inflated again by the small inflater below: the filtered bytes of a straightforward filter loop must come back, and the Adler-32 must match.
#include "../../sudoku-vision_amd/csrc/host_png.cpp"
#include <memory>
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

// RFC 1951 by the book: canonical codes decoded a bit at a time
struct Inflater {
    const uint8_t *p; size_t n, at = 0; uint32_t buf = 0; int cnt = 0; bool bad = false;
    std::vector<uint8_t> out;
    struct Huff { int count[16]; int symbol[320]; };
    int bits(int need)
    {
        while (cnt < need) { if (at >= n) { bad = true; return 0; } buf |= (uint32_t)p[at++] << cnt; cnt += 8; }
        const int v = (int)(buf & ((1u << need) - 1));
        buf >>= need; cnt -= need;
        return v;
    }
    static bool construct(Huff &h, const int *len, int n)
    {
        for (int &c : h.count) c = 0;
        for (int i = 0; i < n; i++) h.count[len[i]]++;
        int left = 1;
        for (int l = 1; l < 16; l++) { left = 2 * left - h.count[l]; if (left < 0) return false; }
        int offs[16]; offs[1] = 0;
        for (int l = 1; l < 15; l++) offs[l + 1] = offs[l] + h.count[l];
        for (int i = 0; i < n; i++) if (len[i]) h.symbol[offs[len[i]]++] = i;
        return left == 0;                                              // complete
    }
    int decode(const Huff &h)
    {
        int code = 0, first = 0, index = 0;
        for (int l = 1; l < 16; l++) {
            code |= bits(1);
            const int c = h.count[l];
            if (code - c < first) return h.symbol[index + (code - first)];
            index += c; first += c; first <<= 1; code <<= 1;
        }
        bad = true;
        return -1;
    }
    bool run()
    {
        static const int lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        static const int lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
        for (;;) {
            const int last = bits(1), type = bits(2);
            if (bad) return false;
            if (type == 0) {
                buf = 0; cnt = 0;
                if (at + 4 > n) return false;
                const int len = p[at] | p[at + 1] << 8, nlen = p[at + 2] | p[at + 3] << 8;
                at += 4;
                if ((len ^ 0xffff) != nlen || at + len > n) return false;
                out.insert(out.end(), p + at, p + at + len);
                at += len;
            } else if (type == 3) return false;
            else {
                Huff lit, dist;
                int len[320];
                if (type == 1) {
                    for (int i = 0; i < 288; i++) len[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
                    construct(lit, len, 288);
                    for (int i = 0; i < 30; i++) len[i] = 5;
                    construct(dist, len, 30);
                } else {
                    static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
                    const int nlen = bits(5) + 257, ndist = bits(5) + 1, ncode = bits(4) + 4;
                    if (nlen > 286 || ndist > 30) return false;
                    int cl[19] = {};
                    for (int i = 0; i < ncode; i++) cl[order[i]] = bits(3);
                    Huff clh;
                    if (!construct(clh, cl, 19)) return false;
                    int i = 0;
                    while (i < nlen + ndist) {
                        const int s = decode(clh);
                        if (bad) return false;
                        if (s < 16) len[i++] = s;
                        else {
                            int prev = 0, rep;
                            if (s == 16) { if (!i) return false; prev = len[i - 1]; rep = 3 + bits(2); }
                            else rep = s == 17 ? 3 + bits(3) : 11 + bits(7);
                            if (i + rep > nlen + ndist) return false;
                            while (rep--) len[i++] = prev;
                        }
                    }
                    if (!len[256]) return false;
                    if (!construct(lit, len, nlen)) return false;      // this encoder's codes are complete
                    if (!construct(dist, len + nlen, ndist)) return false;
                }
                for (;;) {
                    const int s = decode(lit);
                    if (bad) return false;
                    if (s < 256) out.push_back((uint8_t)s);
                    else if (s == 256) break;
                    else {
                        if (s - 257 >= 29) return false;
                        const int l = lbase[s - 257] + bits(lext[s - 257]);
                        const int d = decode(dist);
                        if (bad || d != 0 || out.empty()) return false;   // distance 1 only
                        out.insert(out.end(), (size_t)l, out.back());
                    }
                }
            }
            if (last) return !bad;
        }
    }
};

uint32_t adler32(const std::vector<uint8_t> &v)
{
    uint32_t a = 1, b = 0;
    for (uint8_t x : v) { a = (a + x) % 65521; b = (b + a) % 65521; }
    return b << 16 | a;
}

// the filtered bytes, pixel by pixel; adaptive: smallest sum of abs((int8) byte), lowest number on a tie
std::vector<uint8_t> filtered(const std::vector<uint8_t> &img, int W, int H, int ch, long pitch, int filter)
{
    std::vector<uint8_t> out;
    const int rb = W * ch;
    auto raw = [&](int y, int x) -> int {
        if (y < 0 || x < 0) return 0;
        const int px = x / ch, c = x % ch;
        return img[(size_t)y * pitch + (size_t)px * ch + (ch == 3 ? 2 - c : 0)];
    };
    for (int y = 0; y < H; y++) {
        std::vector<uint8_t> rows[5];
        long sums[5] = {0, 0, 0, 0, 0};
        for (int f = 0; f < 5; f++)
            for (int x = 0; x < rb; x++) {
                const int v = raw(y, x), a = raw(y, x - ch), b = raw(y - 1, x), c = raw(y - 1, x - ch);
                const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
                const int pr = pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
                const uint8_t e = (uint8_t)(f == 0 ? v : f == 1 ? v - a : f == 2 ? v - b : f == 3 ? v - (a + b) / 2 : v - pr);
                rows[f].push_back(e);
                sums[f] += abs((int)(int8_t)e);
            }
        int f = filter;
        if (filter == 5) { f = 0; for (int k = 1; k < 5; k++) if (sums[k] < sums[f]) f = k; }
        out.push_back((uint8_t)f);
        out.insert(out.end(), rows[f].begin(), rows[f].end());
    }
    return out;
}

template <int CAP>
void run_band(const svpng::Geom &g, const uint8_t *img, int band, uint8_t *slot, uint32_t *len, uint32_t *ad, uint32_t *st)
{
    using namespace svpng;
    auto b = std::make_unique<Band<CAP>>();
    std::vector<Lane> L(kThreads);
    const bool back = band & 1;
#define PHASE(call) for (int k = 0; k < kThreads; k++) { const int tid = back ? kThreads - 1 - k : k; call; }
    PHASE(b->p0_init(g, band, tid))
    if (g.filter == kFilterAdaptive) { PHASE(b->p1_row_sums(g, img, tid)) PHASE(b->p2_row_choice(tid)) }
    PHASE(b->p3_filter(g, img, tid))
    PHASE(b->p4_chunks(tid))
    PHASE(b->p5_histogram(g, L[tid], tid))
    if (g.strategy != kStored) { PHASE(b->p6_keys(tid)) PHASE(b->p7_rank(tid)) PHASE(b->p8_code(tid)) PHASE(b->p9_measure(g, L[tid], tid)) }
    PHASE(b->p10_pack(g, L[tid], tid))
    PHASE(b->p11_store(g, slot, len, ad, st, tid))
#undef PHASE
}

std::vector<uint8_t> make_image(std::mt19937 &rng, int kind, int W, int H, int ch, long pitch)
{
    std::vector<uint8_t> img((size_t)H * pitch, 0xA5);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W * ch; x++) {
            uint8_t v = 0;
            switch (kind) {
            case 0: v = 0; break;                                      // all matches
            case 1: v = (uint8_t)rng(); break;                         // no matches: the stored fall-back
            case 2: v = (uint8_t)(x / ch / 7 * 31 + y / 5 * 17); break; // flat patches: runs of many lengths
            case 3: v = (uint8_t)((x / ch + y) * 3 + (rng() % 16 == 0)); break;   // ramps, a little noise
            default: v = (uint8_t)(rng() % 3 == 0 ? rng() : 200); break;          // short runs between literals
            }
            img[(size_t)y * pitch + x] = v;
        }
    return img;
}

}  // namespace

int main(int argc, char **argv)                                        // with a directory: every 37th file is left there, for other decoders
{
    std::mt19937 rng(18);
    long files = 0, bad = 0;
    // 1. the host half alone
    for (int round = 0; round < 200; round++) {
        const int W = 1 + (int)(rng() % 300), H = 1 + (int)(rng() % 200), ch = rng() & 1 ? 3 : 1, rows = (int)(rng() % 9);
        sv_png_enc plan;
        if (sv_png_encode_plan(W, H, ch, (int)(rng() % 6), (int)(rng() % 3), rows, &plan) != SV_OK) { bad++; continue; }
        std::vector<uint32_t> len((size_t)plan.bands), ad((size_t)plan.bands);
        size_t total = 0;
        for (int b = 0; b < plan.bands; b++) {
            const long cap = band_bytes(plan, b) + 10;
            len[b] = (uint32_t)(rng() % 4 == 0 ? cap : rng() % 5 == 0 ? 0 : rng() % (cap + 1));
            ad[b] = (uint32_t)(rng() % 65521) << 16 | (uint32_t)(rng() % 65521);
            total += len[b];
        }
        std::vector<uint8_t> stream(total + 1);
        for (auto &x : stream) x = (uint8_t)rng();
        std::vector<uint8_t> file((size_t)plan.out_bound);
        size_t n1 = 0, n2 = 0;
        if (sv_png_assemble(&plan, stream.data(), len.data(), ad.data(), file.data(), file.size(), &n1) != SV_OK || n1 != total + kContainer) { bad++; continue; }
        std::vector<uint8_t> exact(n1), shorter(n1 - 1);
        if (sv_png_assemble(&plan, stream.data(), len.data(), ad.data(), exact.data(), n1, &n2) != SV_OK || n2 != n1 || memcmp(exact.data(), file.data(), n1) != 0) bad++;
        if (sv_png_assemble(&plan, stream.data(), len.data(), ad.data(), shorter.data(), n1 - 1, &n2) != SV_ERR_BUFFER || n2 != n1) bad++;
        const int which = (int)(rng() % plan.bands);
        const uint32_t keep = len[which];
        len[which] = (uint32_t)band_bytes(plan, which) + 11;
        if (sv_png_assemble(&plan, stream.data(), len.data(), ad.data(), file.data(), file.size(), &n2) != SV_ERR_BAD_ARG) bad++;
        len[which] = keep;
        // the batch: three copies of the frame on 1 and 4 threads
        std::vector<uint8_t> o[2][3];
        for (int t = 0; t < 2; t++) {
            const uint8_t *streams[3]; const uint32_t *lens[3], *ads[3]; uint8_t *outs[3]; size_t caps[3], sizes[3]; int status[3];
            for (int i = 0; i < 3; i++) { o[t][i].resize(n1); streams[i] = stream.data(); lens[i] = len.data(); ads[i] = ad.data(); outs[i] = o[t][i].data(); caps[i] = n1; }
            if (sv_png_assemble_batch(&plan, 3, streams, lens, ads, outs, caps, sizes, t ? 4 : 1, status) != SV_OK) bad++;
            for (int i = 0; i < 3; i++) if (sizes[i] != n1 || memcmp(o[t][i].data(), exact.data(), n1) != 0) bad++;
        }
        files++;
    }
    // 2. the band algorithm
    long bands_run = 0, coded = 0;
    const int sizes[][2] = {{1, 1}, {1, 5}, {7, 5}, {64, 48}, {53, 37}, {1920, 4}, {80, 48}, {700, 3}, {300, 300}, {12000, 2}, {21844, 1}, {2, 1100}};
    for (const auto &wh : sizes)
        for (int ch : {1, 3})
            for (int kind = 0; kind < 5; kind++)
                for (int filter = 0; filter < 6; filter++)
                    for (int strategy = 0; strategy < 3; strategy++)
                        for (int rows : {0, 1, 3}) {
                            const int W = wh[0], H = wh[1];
                            if ((long)W * H > 20000 && (filter % 2 == 0 || strategy == 1 || rows == 1) && kind != 2) continue;      // the large ones on fewer settings
                            if (strategy && (filter != 1 && filter != 5)) continue;
                            sv_png_enc plan;
                            const int rc = sv_png_encode_plan(W, H, ch, filter, strategy, rows, &plan);
                            if (std::min(rows, H) * (1L + (long)W * ch) > svpng::kMaxBandBytes) { bad += rc != SV_ERR_BAD_ARG; continue; }     // too many rows for one band
                            if (rc != SV_OK) { bad++; printf("plan: %d x %d x %d rows %d\n", W, H, ch, rows); continue; }
                            const long pitch = (long)W * ch + (kind == 3 ? 5 : 0);
                            const std::vector<uint8_t> img = make_image(rng, kind, W, H, ch, pitch);
                            svpng::Geom g = {};
                            g.W = W; g.H = H; g.bpp = ch; g.filter = filter; g.strategy = strategy; g.band_rows = plan.band_rows; g.bands = plan.bands;
                            g.row_bytes = (int)plan.row_bytes; g.pitch = pitch; g.frame_stride = 0; g.slot_bytes = plan.slot_bytes;
                            std::vector<uint32_t> len((size_t)plan.bands), ad((size_t)plan.bands), st((size_t)plan.bands);
                            std::vector<uint8_t> stream;
                            for (int b = 0; b < plan.bands; b++) {
                                // a slot of exactly its size, 16-byte aligned: a byte too many is the sanitizer's
                                uint8_t *slot = (uint8_t *)aligned_alloc(16, (size_t)plan.slot_bytes);
                                if ((long)plan.band_rows * plan.row_bytes <= svpng::kSmallBandBytes) run_band<svpng::kSmallBandBytes>(g, img.data(), b, slot, &len[b], &ad[b], &st[b]);
                                else run_band<svpng::kMaxBandBytes>(g, img.data(), b, slot, &len[b], &ad[b], &st[b]);
                                if (st[b] || len[b] > band_bytes(plan, b) + 5) { bad++; printf("band %d: status %u, %u bytes\n", b, st[b], len[b]); }
                                else if (strategy != SV_PNG_STORED && len[b] < band_bytes(plan, b) + 5) coded++;
                                stream.insert(stream.end(), slot, slot + len[b]);
                                free(slot);
                                bands_run++;
                            }
                            stream.push_back(0);
                            std::vector<uint8_t> file((size_t)plan.out_bound);
                            size_t n = 0;
                            if (sv_png_assemble(&plan, stream.data(), len.data(), ad.data(), file.data(), file.size(), &n) != SV_OK) { bad++; continue; }
                            const std::vector<uint8_t> want = filtered(img, W, H, ch, pitch, filter);
                            Inflater z{file.data() + 8 + 25 + 8 + 2, n - (8 + 25 + 8 + 2) - 4 - 4 - 12};
                            if (!z.run() || z.at != z.n || z.out != want) { bad++; printf("mismatch: %d x %d x %d kind %d filter %d strategy %d rows %d\n", W, H, ch, kind, filter, strategy, rows); continue; }
                            const uint8_t *a = file.data() + n - 12 - 4 - 4;
                            if (((uint32_t)a[0] << 24 | a[1] << 16 | a[2] << 8 | a[3]) != adler32(want)) { bad++; printf("adler: %d x %d x %d\n", W, H, ch); }
                            if (argc > 1 && files % 37 == 0) {
                                const std::string path = std::string(argv[1]) + "/" + std::to_string(files) + ".png";
                                if (FILE *fp = fopen(path.c_str(), "wb")) { fwrite(file.data(), 1, n, fp); fclose(fp); }
                            }
                            files++;
                        }
    printf("%ld files, %ld bands (%ld coded), %ld checks failed\n", files, bands_run, coded, bad);
    return bad != 0;
}
