// Host-side check of the JPEG encoder's host half (csrc/host_jpeg.cpp: sv_jpeg_encode_plan, sv_jpeg_entropy_encode, _batch) under AddressSanitizer + UBSan
// (host code only):
//   hipcc -O1 -g -std=c++17 -ffp-contract=off -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
//         -I sudoku-vision_amd/csrc tools/dev/jpeg_encode_asan.cpp -o /tmp/jpeg_encode_asan -lpthread && /tmp/jpeg_encode_asan
// Random sparse records of many shapes, samplings, densities and restart intervals are packed with 1 and 4 threads (the bytes must agree), decoded
// again by the decoder of the same file (sv_jpeg_entropy_decode_sparse: masks and values must come back), packed into a buffer of exactly the size
// reported, and refused when the buffer is a byte short or the records are malformed.
#include "../../sudoku-vision_amd/csrc/host_jpeg.cpp"
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

int main()
{
    std::mt19937 rng(17);
    long files = 0, bad = 0;
    const int sizes[][2] = {{1, 1}, {8, 8}, {17, 33}, {33, 17}, {100, 7}, {64, 48}, {130, 70}};
    for (const auto &wh : sizes)
        for (int comps : {1, 3})
            for (int sampling : {SV_JPEG_444, SV_JPEG_422, SV_JPEG_420})
                for (int restart : {0, 1, 3})
                    for (int density : {0, 3, 40, 64}) {
                        if (comps == 1 && sampling != SV_JPEG_444) continue;
                        sv_jpeg_enc plan;
                        if (sv_jpeg_encode_plan(wh[0], wh[1], comps, sampling, 75, restart, &plan) != SV_OK) { bad++; continue; }
                        const long nb = plan.info.coef_count / 64;
                        std::vector<uint64_t> masks((size_t)nb);
                        std::vector<uint32_t> offsets((size_t)nb);
                        std::vector<int16_t> values;
                        int dc = 0;
                        for (long b = 0; b < nb; b++) {
                            offsets[b] = (uint32_t)values.size();
                            uint64_t m = 0;
                            dc = std::max(-1000, std::min(1000, dc + (int)(rng() % 201) - 100));   // DC differences stay within 11 bits
                            if (dc) { m |= 1; values.push_back((int16_t)dc); }
                            for (int k = 1; k < 64; k++)
                                if ((int)(rng() % 64) < density) {
                                    const int mag = 1 + (int)(rng() % (k < 4 ? 1023 : 31));
                                    m |= 1ull << k;
                                    values.push_back((int16_t)((rng() & 1) ? mag : -mag));
                                }
                            masks[b] = m;
                        }
                        values.push_back(0);                                                       // never an empty buffer
                        const long count = (long)values.size() - 1;
                        const long cap = sv_jpeg_encode_bound(&plan, count);
                        std::vector<uint8_t> a((size_t)cap), b4((size_t)cap);
                        size_t na = 0, nb4 = 0;
                        if (sv_jpeg_entropy_encode(&plan, masks.data(), offsets.data(), values.data(), count, a.data(), a.size(), &na, 1) != SV_OK) { bad++; continue; }
                        if (sv_jpeg_entropy_encode(&plan, masks.data(), offsets.data(), values.data(), count, b4.data(), b4.size(), &nb4, 4) != SV_OK || na != nb4 ||
                            memcmp(a.data(), b4.data(), na) != 0) bad++;
                        std::vector<uint8_t> exact(na), shorter(na - 1);
                        size_t n2 = 0;
                        if (sv_jpeg_entropy_encode(&plan, masks.data(), offsets.data(), values.data(), count, exact.data(), na, &n2, 1) != SV_OK || n2 != na) bad++;
                        if (sv_jpeg_entropy_encode(&plan, masks.data(), offsets.data(), values.data(), count, shorter.data(), na - 1, &n2, 1) != SV_ERR_BUFFER || n2 != na) bad++;
                        if (count > 2 && sv_jpeg_entropy_encode(&plan, masks.data(), offsets.data(), values.data(), count - 2, a.data(), a.size(), &n2, 1) != SV_ERR_BAD_ARG) bad++;
                        // the decoder of this file reads the records back
                        sv_jpeg_info info;
                        if (sv_jpeg_parse(exact.data(), na, &info) != SV_OK || info.coef_count != plan.info.coef_count || info.restart_interval != restart) { bad++; continue; }
                        std::vector<uint64_t> m2((size_t)nb);
                        std::vector<uint32_t> o2((size_t)nb);
                        std::vector<int16_t> v2((size_t)info.sparse_capacity + 1);
                        uint16_t quant[192];
                        long used = 0;
                        if (sv_jpeg_entropy_decode_sparse(exact.data(), na, m2.data(), o2.data(), v2.data(), info.sparse_capacity, &used, quant, 2) != SV_OK) { bad++; continue; }
                        for (long blk = 0; blk < nb; blk++) {
                            if (m2[blk] != masks[blk]) { bad++; break; }
                            if (memcmp(v2.data() + o2[blk], values.data() + offsets[blk], 2 * (size_t)__builtin_popcountll(masks[blk])) != 0) { bad++; break; }
                        }
                        if (memcmp(quant, plan.quant, 2 * 64 * (size_t)comps) != 0) bad++;
                        files++;
                    }
    printf("%ld files packed and read back, %ld checks failed\n", files, bad);
    return bad != 0;
}
