// Host half of the PNG encoder: the plan (geometry, bands, bounds) and the container.  The device half (k18_png_encode.hip) leaves a frame as the deflate
// streams of its bands, each a whole number of bytes, and the Adler-32 of each band's filtered bytes; what remains is the signature, IHDR, the
// IDAT chunk (zlib header 78 01, the bands, the final empty fixed block 03 00, the combined Adler-32), IEND and the chunks' CRC-32s.  No libz, no
// libpng.
#include <cstring>
#include <string>

#include "host_pool.h"
#include "sv_internal.h"
#include "sv_png_band.h"

namespace {

// CRC-32 (ISO 3309, polynomial edb88320), eight table look-ups per eight bytes
struct CrcTables {
    uint32_t t[8][256];
    CrcTables()
    {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = c & 1 ? 0xedb88320u ^ (c >> 1) : c >> 1;
            t[0][i] = c;
        }
        for (int j = 1; j < 8; j++)
            for (uint32_t i = 0; i < 256; i++) t[j][i] = t[0][t[j - 1][i] & 0xff] ^ (t[j - 1][i] >> 8);
    }
};
const CrcTables &crc_tables() { static const CrcTables c; return c; }

uint32_t crc32_update(uint32_t crc, const uint8_t *p, size_t n)
{
    const auto &t = crc_tables().t;
    crc = ~crc;
    while (n >= 8) {
        uint32_t a, b;
        memcpy(&a, p, 4); memcpy(&b, p + 4, 4);                     // little-endian hosts only (so is the rest of this library)
        a ^= crc;
        crc = t[7][a & 0xff] ^ t[6][(a >> 8) & 0xff] ^ t[5][(a >> 16) & 0xff] ^ t[4][a >> 24] ^ t[3][b & 0xff] ^ t[2][(b >> 8) & 0xff] ^ t[1][(b >> 16) & 0xff] ^ t[0][b >> 24];
        p += 8; n -= 8;
    }
    while (n--) crc = t[0][(crc ^ *p++) & 0xff] ^ (crc >> 8);
    return ~crc;
}

void be32(uint8_t *o, uint32_t v) { o[0] = (uint8_t)(v >> 24); o[1] = (uint8_t)(v >> 16); o[2] = (uint8_t)(v >> 8); o[3] = (uint8_t)v; }

long band_bytes(const sv_png_enc &p, int band)
{
    const long rows = std::min<long>(p.band_rows, p.height - (long)band * p.band_rows);
    return rows * p.row_bytes;
}

bool plan_ok(const sv_png_enc *p)
{
    sv_png_enc want;
    return p && sv_png_encode_plan(p->width, p->height, p->channels, p->filter, p->strategy, p->band_rows, &want) == SV_OK && want.bands == p->bands &&
           want.band_rows == p->band_rows && want.row_bytes == p->row_bytes && want.filtered_bytes == p->filtered_bytes && want.slot_bytes == p->slot_bytes &&
           want.stream_bound == p->stream_bound && want.out_bound == p->out_bound;
}

constexpr size_t kContainer = 8 + 25 + 12 + 2 + 2 + 4 + 12;           // signature, IHDR, IDAT's frame, zlib header, final block, Adler-32, IEND

int assemble(const sv_png_enc &p, const uint8_t *stream, const uint32_t *band_len, const uint32_t *adler, uint8_t *out, size_t out_cap, size_t *out_size)
{
    size_t total = 0;
    uint32_t A = 1, B = 0;                                            // Adler-32 of the bands one after the other
    for (int b = 0; b < p.bands; b++) {
        const long n = band_bytes(p, b);
        if ((long)band_len[b] > n + 10) return sv_fail(SV_ERR_BAD_ARG, "png assemble: band %d has %u bytes, its bound is %ld", b, band_len[b], n + 10);
        total += band_len[b];
        const uint32_t a2 = adler[b] & 0xffff, b2 = adler[b] >> 16;
        if (a2 >= svpng::kAdlerBase || b2 >= svpng::kAdlerBase) return sv_fail(SV_ERR_BAD_ARG, "png assemble: band %d: %08x is not an Adler-32", b, adler[b]);
        const uint32_t rem = (uint32_t)(n % svpng::kAdlerBase);
        B = (uint32_t)((B + (uint64_t)rem * A + b2 + svpng::kAdlerBase - rem) % svpng::kAdlerBase);      // b2 counts its own start value 1 n times
        A = (A + a2 + svpng::kAdlerBase - 1) % svpng::kAdlerBase;
    }
    const size_t idat = 2 + total + 2 + 4, need = kContainer + total;
    *out_size = need;
    if (idat > 0x7fffffffu) return sv_fail(SV_ERR_UNSUPPORTED, "png assemble: %zu bytes do not fit one IDAT chunk", idat);
    if (need > out_cap) return sv_fail(SV_ERR_BUFFER, "png assemble: the file takes %zu bytes, the buffer holds %zu", need, out_cap);
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    uint8_t *o = out;
    memcpy(o, sig, 8); o += 8;
    be32(o, 13); memcpy(o + 4, "IHDR", 4);
    be32(o + 8, (uint32_t)p.width); be32(o + 12, (uint32_t)p.height);
    o[16] = 8; o[17] = p.channels == 3 ? 2 : 0; o[18] = 0; o[19] = 0; o[20] = 0;
    be32(o + 21, crc32_update(0, o + 4, 17)); o += 25;
    be32(o, (uint32_t)idat); memcpy(o + 4, "IDAT", 4);
    uint8_t *z = o + 8;
    z[0] = 0x78; z[1] = 0x01;
    if (total) memcpy(z + 2, stream, total);
    z[2 + total] = 0x03; z[3 + total] = 0x00;
    be32(z + 4 + total, B << 16 | A);
    be32(o + 8 + idat, crc32_update(0, o + 4, 4 + idat)); o += 12 + idat;
    be32(o, 0); memcpy(o + 4, "IEND", 4); be32(o + 8, crc32_update(0, o + 4, 4));
    return SV_OK;
}

}  // namespace

extern "C" int sv_png_encode_plan(int width, int height, int channels, int filter, int strategy, int band_rows, sv_png_enc *plan)
{
    if (!plan) return sv_fail(SV_ERR_BAD_ARG, "sv_png_encode_plan: NULL argument");
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535) return sv_fail(SV_ERR_BAD_ARG, "sv_png_encode_plan: size %d x %d (1..65535)", width, height);
    if (channels != 1 && channels != 3) return sv_fail(SV_ERR_BAD_ARG, "sv_png_encode_plan: %d channels (1 or 3)", channels);
    if (filter < SV_PNG_FILTER_NONE || filter > SV_PNG_FILTER_ADAPTIVE) return sv_fail(SV_ERR_BAD_ARG, "sv_png_encode_plan: unknown filter %d", filter);
    if (strategy < SV_PNG_RLE || strategy > SV_PNG_STORED) return sv_fail(SV_ERR_BAD_ARG, "sv_png_encode_plan: unknown strategy %d", strategy);
    if (band_rows < 0 || band_rows > svpng::kMaxRows) return sv_fail(SV_ERR_BAD_ARG, "sv_png_encode_plan: band_rows %d (0 = automatic, 1..%d)", band_rows, svpng::kMaxRows);
    const long row = 1 + (long)width * channels;
    if (row > svpng::kMaxBandBytes) return sv_fail(SV_ERR_UNSUPPORTED, "sv_png_encode_plan: a row of %ld filtered bytes (at most %d)", row, svpng::kMaxBandBytes);
    long rows = band_rows;
    if (rows == 0) {
        rows = (32768 + row - 1) / row;
        if (rows * row > svpng::kSmallBandBytes) rows = std::max(1L, svpng::kSmallBandBytes / row);
        rows = std::min<long>(rows, svpng::kMaxRows);
    }
    rows = std::min<long>(rows, height);
    if (rows * row > svpng::kMaxBandBytes) return sv_fail(SV_ERR_BAD_ARG, "sv_png_encode_plan: %ld rows of %ld bytes are more than a band's %d", rows, row, svpng::kMaxBandBytes);
    memset(plan, 0, sizeof *plan);
    plan->width = width; plan->height = height; plan->channels = channels; plan->filter = filter; plan->strategy = strategy;
    plan->band_rows = (int)rows;
    plan->bands = (int)((height + rows - 1) / rows);
    plan->row_bytes = row;
    plan->filtered_bytes = row * height;
    plan->slot_bytes = (rows * row + 10 + 15) / 16 * 16;
    plan->stream_bound = plan->filtered_bytes + 10L * plan->bands;
    plan->out_bound = plan->stream_bound + (long)kContainer;
    return SV_OK;
}

extern "C" int sv_png_assemble(const sv_png_enc *plan, const uint8_t *stream, const uint32_t *band_len, const uint32_t *adler, uint8_t *out, size_t out_cap, size_t *out_size)
{
    if (!plan || !stream || !band_len || !adler || !out || !out_size) return sv_fail(SV_ERR_BAD_ARG, "sv_png_assemble: NULL argument");
    if (!plan_ok(plan)) return sv_fail(SV_ERR_BAD_ARG, "sv_png_assemble: the plan was not made by sv_png_encode_plan");
    return assemble(*plan, stream, band_len, adler, out, out_cap, out_size);
}

extern "C" int sv_png_assemble_batch(const sv_png_enc *plan, int n, const uint8_t *const *streams, const uint32_t *const *band_len, const uint32_t *const *adler,
                                     uint8_t *const *outs, const size_t *out_caps, size_t *out_sizes, int threads, int *status)
{
    if (!plan || !streams || !band_len || !adler || !outs || !out_caps || !out_sizes || !status || n <= 0) return sv_fail(SV_ERR_BAD_ARG, "sv_png_assemble_batch: bad argument");
    if (!plan_ok(plan)) return sv_fail(SV_ERR_BAD_ARG, "sv_png_assemble_batch: the plan was not made by sv_png_encode_plan");
    auto one = [&](int i) {
        out_sizes[i] = 0;
        const bool ok = streams[i] && band_len[i] && adler[i] && outs[i];
        status[i] = ok ? assemble(*plan, streams[i], band_len[i], adler[i], outs[i], out_caps[i], out_sizes + i) : SV_ERR_BAD_ARG;
    };
    WorkerPool::instance().parallel_for(n, threads < 1 ? 1 : threads, one);
    for (int i = 0; i < n; i++)
        if (status[i] != SV_OK) return sv_fail(status[i], "sv_png_assemble_batch: image %d failed (see status[])", i);
    return SV_OK;
}
