// Host-side check of the luma-only mode of the JPEG entropy decoder (csrc/host_jpeg.cpp: sv_jpeg_parse_luma, sv_jpeg_entropy_decode_luma, _luma_sparse,
// _luma_batch) under AddressSanitizer + UBSan (host code only):
//   hipcc -O1 -g -std=c++17 -ffp-contract=off -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
//         -I sudoku-vision_amd/csrc tools/dev/jpeg_luma_asan.cpp -o /tmp/jpeg_luma_asan -lpthread && /tmp/jpeg_luma_asan
// Files of many shapes, samplings, densities and restart intervals are written by the encoder of the same source file from random records, then
// decoded luma-only into heap buffers of EXACTLY the sizes sv_jpeg_parse_luma states (a write past any of them is an ASan report): the valid file
// (Y's blocks must be the records that were written, and what the full decode returns), every truncation of it, and a sweep of single-byte
// flips.  Whatever the full decode answers for a damaged stream -- a status, or blocks -- the luma mode must answer too.
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

struct Counts { long valid = 0, truncations = 0, flips = 0, refused = 0, bad = 0; };

// Y's blocks of the full decode (component 0: raster over its padded grid) in the luma records' order
static std::vector<int16_t> luma_of_full(const sv_jpeg_info &f, const std::vector<int16_t> &coef)
{
    const int hs = f.h_samp, vs = f.v_samp, mcu_cols = (f.width + 8 * hs - 1) / (8 * hs), mcu_rows = (f.height + 8 * vs - 1) / (8 * vs), bw = mcu_cols * hs;
    std::vector<int16_t> out((size_t)64 * bw * mcu_rows * vs);
    for (int by = 0; by < mcu_rows * vs; by++)
        for (int bx = 0; bx < bw; bx++) {
            const long rec = ((long)(by / vs) * mcu_cols + bx / hs) * hs * vs + (by % vs) * hs + bx % hs;
            memcpy(out.data() + 64 * rec, coef.data() + 64 * ((long)by * bw + bx), 128);
        }
    return out;
}

// One stream through both modes, dense and compact, in exact buffers.  Returns the luma mode's status.
static int both_modes(const uint8_t *d, size_t n, Counts &c, int threads)
{
    sv_jpeg_info full, luma;
    const int pf = sv_jpeg_parse(d, n, &full), pl = sv_jpeg_parse_luma(d, n, &luma);
    if (pf != pl) { c.bad++; return pl; }
    if (pf) return pf;
    if (luma.coef_count != 64L * ((full.width + 8 * full.h_samp - 1) / (8 * full.h_samp)) * ((full.height + 8 * full.v_samp - 1) / (8 * full.v_samp)) * full.h_samp * full.v_samp ||
        luma.sparse_capacity > luma.coef_count || luma.coef_count > full.coef_count) c.bad++;
    std::vector<int16_t> fc((size_t)full.coef_count), lc((size_t)luma.coef_count);
    std::vector<uint16_t> fq(192), lq(64);
    const int rf = sv_jpeg_entropy_decode(d, n, fc.data(), fq.data(), threads);
    const std::string mf = rf ? g_msg : "";
    const int rl = sv_jpeg_entropy_decode_luma(d, n, lc.data(), lq.data(), threads);
    if (rf != rl || (rf && mf != g_msg)) c.bad++;
    if (!rf && !rl && (luma_of_full(full, fc) != lc || memcmp(fq.data(), lq.data(), 128) != 0)) c.bad++;
    const size_t nb = (size_t)luma.coef_count / 64;
    std::vector<uint64_t> masks(nb);
    std::vector<uint32_t> offs(nb);
    std::vector<int16_t> vals((size_t)luma.sparse_capacity);
    long used = -1;
    const int rs = sv_jpeg_entropy_decode_luma_sparse(d, n, masks.data(), offs.data(), vals.data(), luma.sparse_capacity, &used, lq.data(), threads);
    if (rs != rl || used > luma.sparse_capacity) c.bad++;
    if (!rs && !rl)
        for (size_t b = 0; b < nb; b++) {                       // the compact records expand to the dense blocks
            int16_t blk[64] = {0};
            long at = offs[b];
            for (int z = 0; z < 64; z++)
                if (masks[b] >> z & 1) {
                    if (at >= used) { c.bad++; break; }
                    blk[kNatural[z]] = vals[(size_t)at++];
                }
            if (memcmp(blk, lc.data() + 64 * b, 128) != 0) { c.bad++; break; }
        }
    return rl;
}

int main()
{
    std::mt19937 rng(23);
    Counts c;
    const int sizes[][2] = {{1, 1}, {7, 5}, {8, 8}, {9, 9}, {16, 16}, {17, 17}, {33, 17}, {53, 37}, {100, 7}};
    std::vector<std::vector<uint8_t>> keep;                     // a few files for the batch entry
    for (const auto &wh : sizes)
        for (int comps : {1, 3})
            for (int sampling : {SV_JPEG_444, SV_JPEG_422, SV_JPEG_420})
                for (int restart : {0, 1, 3})
                    for (int density : {0, 6, 64}) {
                        if (comps == 1 && sampling != SV_JPEG_444) continue;
                        sv_jpeg_enc plan;
                        if (sv_jpeg_encode_plan(wh[0], wh[1], comps, sampling, 75, restart, &plan) != SV_OK) { c.bad++; continue; }
                        const long nb = plan.info.coef_count / 64;
                        std::vector<uint64_t> masks((size_t)nb);
                        std::vector<uint32_t> offsets((size_t)nb);
                        std::vector<int16_t> values;
                        int dc = 0;
                        for (long b = 0; b < nb; b++) {
                            offsets[b] = (uint32_t)values.size();
                            uint64_t m = 0;
                            dc = std::max(-1000, std::min(1000, dc + (int)(rng() % 201) - 100));
                            if (dc) { m |= 1; values.push_back((int16_t)dc); }
                            for (int k = 1; k < 64; k++)
                                if ((int)(rng() % 64) < density) {
                                    const int mag = 1 + (int)(rng() % (k < 4 ? 1023 : 31));
                                    m |= 1ull << k;
                                    values.push_back((int16_t)((rng() & 1) ? mag : -mag));
                                }
                            masks[b] = m;
                        }
                        values.push_back(0);
                        const long count = (long)values.size() - 1;
                        std::vector<uint8_t> file((size_t)sv_jpeg_encode_bound(&plan, count));
                        size_t n = 0;
                        if (sv_jpeg_entropy_encode(&plan, masks.data(), offsets.data(), values.data(), count, file.data(), file.size(), &n, 1) != SV_OK) { c.bad++; continue; }
                        file.resize(n);
                        // the valid file: Y's records are the first component's records that were written
                        if (both_modes(file.data(), n, c, 1) != SV_OK || both_modes(file.data(), n, c, 3) != SV_OK) c.bad++;
                        {
                            sv_jpeg_info luma;
                            uint16_t q[64];
                            std::vector<int16_t> lc;
                            if (sv_jpeg_parse_luma(file.data(), n, &luma) == SV_OK) {
                                lc.resize((size_t)luma.coef_count);
                                if (sv_jpeg_entropy_decode_luma(file.data(), n, lc.data(), q, 1) != SV_OK) c.bad++;
                                std::vector<int16_t> fullc((size_t)plan.info.coef_count, 0);
                                for (long b = 0; b < luma.coef_count / 64; b++) {                  // component 0 comes first in the records
                                    long at = offsets[b];
                                    for (int z = 0; z < 64; z++)
                                        if (masks[b] >> z & 1) fullc[(size_t)(64 * b + kNatural[z])] = values[(size_t)at++];
                                }
                                if (luma_of_full(plan.info, fullc) != lc) c.bad++;
                            } else c.bad++;
                        }
                        c.valid++;
                        if (keep.size() < 12 && density == 6) keep.push_back(file);
                        // every truncation (of the small files; of the others every 7th length), from an exact-size copy so that a read past the cut is a report too
                        const size_t step = n > 1500 ? 7 : 1;
                        for (size_t cut = 0; cut < n; cut += step) {
                            std::vector<uint8_t> part(file.begin(), file.begin() + (long)cut);
                            part.shrink_to_fit();
                            if (both_modes(part.data(), cut, c, 1 + (int)(cut & 1)) != SV_OK) c.refused++;
                            c.truncations++;
                        }
                        // single-byte flips: every header byte of the small files, then a sweep through the rest
                        for (size_t at = 2; at < n; at += (at < 700 && n < 1500) ? 1 : 1 + rng() % 37) {
                            std::vector<uint8_t> dmg(file);
                            dmg[at] ^= (uint8_t)(1u << (rng() % 8));
                            if (both_modes(dmg.data(), n, c, 1) != SV_OK) c.refused++;
                            c.flips++;
                        }
                    }
    // the batch entry: exact buffers again, dense then compact, one refused image among the good ones
    {
        std::vector<std::vector<uint8_t>> files(keep);
        files.push_back(std::vector<uint8_t>{0xFF, 0xD8, 0xFF, 0xC2, 0x00, 0x0B, 8, 0, 8, 0, 8, 1, 1, 0x11, 0});       // a progressive frame header
        const int n = (int)files.size();
        std::vector<sv_jpeg_info> infos((size_t)n);
        std::vector<std::vector<int16_t>> coefs((size_t)n), vals((size_t)n);
        std::vector<std::vector<uint64_t>> masks((size_t)n);
        std::vector<std::vector<uint32_t>> offs((size_t)n);
        std::vector<const uint8_t *> datas;
        std::vector<size_t> sizes_;
        std::vector<int16_t *> cp, vp;
        std::vector<uint64_t *> mp;
        std::vector<uint32_t *> op;
        std::vector<long> caps((size_t)n), used((size_t)n);
        for (int i = 0; i < n; i++) {
            if (sv_jpeg_parse_luma(files[i].data(), files[i].size(), &infos[i]) != SV_OK) { infos[i].coef_count = 64; infos[i].sparse_capacity = 64; }
            coefs[i].resize((size_t)infos[i].coef_count); vals[i].resize((size_t)infos[i].sparse_capacity);
            masks[i].resize((size_t)infos[i].coef_count / 64); offs[i].resize((size_t)infos[i].coef_count / 64);
            datas.push_back(files[i].data()); sizes_.push_back(files[i].size());
            cp.push_back(coefs[i].data()); vp.push_back(vals[i].data()); mp.push_back(masks[i].data()); op.push_back(offs[i].data());
            caps[i] = infos[i].sparse_capacity;
        }
        std::vector<uint16_t> quants((size_t)64 * n);
        std::vector<int> status((size_t)n);
        for (int threads : {1, 4}) {
            if (sv_jpeg_entropy_decode_luma_batch(datas.data(), sizes_.data(), n, cp.data(), nullptr, nullptr, nullptr, nullptr, nullptr, quants.data(), threads, status.data()) !=
                SV_ERR_UNSUPPORTED) c.bad++;
            if (sv_jpeg_entropy_decode_luma_batch(datas.data(), sizes_.data(), n, nullptr, mp.data(), op.data(), vp.data(), caps.data(), used.data(), quants.data(), threads,
                                                  status.data()) != SV_ERR_UNSUPPORTED) c.bad++;
            for (int i = 0; i < n; i++)
                if (status[i] != (i == n - 1 ? SV_ERR_UNSUPPORTED : SV_OK)) c.bad++;
        }
    }
    printf("%ld valid files, %ld truncations, %ld byte flips decoded luma-only in exact buffers (%ld damaged streams refused, by both modes alike); %ld checks failed\n",
           c.valid, c.truncations, c.flips, c.refused, c.bad);
    return c.bad != 0;
}
