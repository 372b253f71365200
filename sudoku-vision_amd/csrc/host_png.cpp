// Host halves of the PNG codec.  Encoder: the plan (geometry, bands, bounds) and the container.  The device half (k18_png_encode.hip) leaves a frame as the deflate
// streams of its bands, each a whole number of bytes, and the Adler-32 of each band's filtered bytes; what remains is the signature, IHDR, the
// IDAT chunk (zlib header 78 01, the bands, the final empty fixed block 03 00, the combined Adler-32), IEND and the chunks' CRC-32s.  No libz, no
// libpng.
// Decoder (second half of this file): the container's parser and the inflater.  The IDAT payloads are read in place as one zlib stream; the device
// half (k19_png_decode.hip) takes the filtered bytes from there.
#include <cstring>
#include <memory>
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

// ---- decoder ---------------------------------------------------------------------------------------------------------------------------------------
namespace {

uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3]; }

int png_channels(int type) { return type == 0 ? 1 : type == 2 ? 3 : type == 3 ? 1 : type == 4 ? 2 : type == 6 ? 4 : 0; }

bool png_depth_ok(int type, int depth)
{
    if (type == 0) return depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
    if (type == 3) return depth == 1 || depth == 2 || depth == 4 || depth == 8;
    return depth == 8 || depth == 16;
}

// The geometry fields that follow from IHDR's five
void png_derive(sv_png_info *info)
{
    info->channels = png_channels(info->color_type);
    const long bits = (long)info->channels * info->bit_depth;
    info->bpp = bits >= 8 ? (int)(bits / 8) : 1;
    info->row_bytes = ((long)info->width * bits + 7) / 8;
    info->filtered_bytes = (long)info->height * (1 + info->row_bytes);
}

// The IDAT payloads from info->idat_offset on as one stream of bits, LSB first; every chunk header is bounds-checked again (the info may not be
// this file's), no byte is copied
struct BitIn {
    const uint8_t *d; size_t size, at;
    const uint8_t *p = nullptr, *end = nullptr;
    uint64_t buf = 0; int nbits = 0;
    BitIn(const uint8_t *data, size_t n, size_t first) : d(data), size(n), at(first) {}
    bool next_chunk()
    {
        for (;;) {
            if (at > size || size - at < 12) return false;
            const uint32_t len = rd32(d + at);
            if (memcmp(d + at + 4, "IDAT", 4) != 0 || len > size - at - 12) return false;
            p = d + at + 8; end = p + len; at += 12 + (size_t)len;
            if (len) return true;
        }
    }
    void refill()
    {
        if (end - p >= 8) {
            uint64_t w;
            memcpy(&w, p, 8);
            buf |= w << nbits;
            p += (63 - nbits) >> 3;
            nbits |= 56;
            buf &= (1ull << nbits) - 1;                               // nbits <= 63: nothing above it but zeros
            return;
        }
        while (nbits <= 56) {
            if (p == end && !next_chunk()) break;
            buf |= (uint64_t)*p++ << nbits;
            nbits += 8;
        }
    }
    bool take(int n, uint32_t &v)                                     // n <= 16
    {
        if (nbits < n) { refill(); if (nbits < n) return false; }
        v = (uint32_t)(buf & ((1u << n) - 1));
        buf >>= n; nbits -= n;
        return true;
    }
    void align() { const int drop = nbits & 7; buf >>= drop; nbits -= drop; }
    bool read_bytes(uint8_t *dst, size_t n)                           // after align()
    {
        while (n && nbits >= 8) { *dst++ = (uint8_t)buf; buf >>= 8; nbits -= 8; n--; }
        while (n) {
            if (p == end && !next_chunk()) return false;
            const size_t k = std::min<size_t>(n, (size_t)(end - p));
            memcpy(dst, p, k);
            dst += k; p += k; n -= k;
        }
        return true;
    }
};

// Two-level decoding tables.  An entry is 0 (no code), symbol << 8 | code bits left to consume, or offset << 8 | 0x80 | index bits of a second-level
// table.  Every second-level table has max - root index bits, so the sizes below hold whatever the code.
constexpr int kLitRoot = 10, kDistRoot = 8, kCodesRoot = 7;
constexpr int kLitTable = (1 << kLitRoot) + 288 * 32, kDistTable = (1 << kDistRoot) + 32 * 128;
struct InflateTables { uint32_t lit[kLitTable], dist[kDistTable], codes[1 << kCodesRoot]; };

enum { kHuffOk = 0, kHuffOver = 1, kHuffIncomplete = 2 };

int build_table(const uint8_t *lens, int n, int root, bool codes, uint32_t *tab, int cap)
{
    int count[16] = {0}, offs[16];
    uint16_t sorted[288];
    for (int i = 0; i < n; i++) count[lens[i]]++;
    count[0] = 0;
    int max = 15;
    while (max > 0 && !count[max]) max--;
    memset(tab, 0, sizeof(uint32_t) << root);
    if (max == 0) return kHuffOk;                                      // no code at all: every look-up fails, as in zlib
    int left = 1;
    for (int l = 1; l <= 15; l++) {
        left = 2 * left - count[l];
        if (left < 0) return kHuffOver;
    }
    if (left > 0 && (codes || max != 1)) return kHuffIncomplete;       // zlib accepts the incomplete code of one 1-bit symbol
    offs[1] = 0;
    for (int l = 1; l < 15; l++) offs[l + 1] = offs[l] + count[l];
    for (int i = 0; i < n; i++)
        if (lens[i]) sorted[offs[lens[i]]++] = (uint16_t)i;
    const int sub_bits = max - root;
    int next = 1 << root, at = 0;
    unsigned code = 0;
    for (int l = 1; l <= max; l++, code <<= 1) {
        for (int k = 0; k < count[l]; k++, code++) {
            unsigned rev = 0;
            for (int b = 0; b < l; b++) rev |= ((code >> b) & 1u) << (l - 1 - b);
            const uint32_t sym = sorted[at++];
            if (l <= root) {
                for (unsigned j = rev; j < (1u << root); j += 1u << l) tab[j] = sym << 8 | (uint32_t)l;
                continue;
            }
            const unsigned first = rev & ((1u << root) - 1);
            if (!tab[first]) {
                if (next + (1 << sub_bits) > cap) return kHuffOver;    // cannot happen: one table per long code at most
                memset(tab + next, 0, sizeof(uint32_t) << sub_bits);
                tab[first] = (uint32_t)next << 8 | 0x80u | (uint32_t)sub_bits;
                next += 1 << sub_bits;
            }
            uint32_t *sub = tab + (tab[first] >> 8);
            for (unsigned j = rev >> root; j < (1u << sub_bits); j += 1u << (l - root)) sub[j] = sym << 8 | (uint32_t)(l - root);
        }
    }
    return kHuffOk;
}

// One symbol from a refilled buffer: 0, or why not
inline const char *decode_symbol(BitIn &in, const uint32_t *tab, int root, uint32_t &sym)
{
    uint32_t e = tab[in.buf & ((1u << root) - 1)];
    int used = 0;
    if (e & 0x80u) {
        e = tab[(e >> 8) + ((in.buf >> root) & ((1u << (e & 0x7f)) - 1))];
        used = root;
    }
    const int len = used + (int)(e & 0x7f);
    if (!e) return in.nbits < 15 ? "truncated input" : "a bit pattern that is no code";
    if (len > in.nbits) return "truncated input";
    in.buf >>= len; in.nbits -= len;
    sym = e >> 8;
    return nullptr;
}

inline const char *take_extra(BitIn &in, int n, uint32_t &v)          // n <= 13, no refill: the caller's refill covers a whole length / distance pair
{
    if (in.nbits < n) return "truncated input";
    v = (uint32_t)(in.buf & ((1u << n) - 1));
    in.buf >>= n; in.nbits -= n;
    return nullptr;
}

uint32_t adler32(const uint8_t *p, size_t n)
{
    uint32_t a = 1, b = 0;
    while (n) {
        size_t k = std::min<size_t>(n, 5552);
        n -= k;
        while (k--) { a += *p++; b += a; }
        a %= svpng::kAdlerBase; b %= svpng::kAdlerBase;
    }
    return b << 16 | a;
}

const char *read_dynamic(BitIn &in, InflateTables &T)
{
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t hlit, hdist, hclen, v;
    if (!in.take(5, hlit) || !in.take(5, hdist) || !in.take(4, hclen)) return "truncated input";
    hlit += 257; hdist += 1; hclen += 4;
    if (hlit > 286 || hdist > 30) return "too many length or distance codes";
    uint8_t cl[19] = {0}, lens[286 + 30];
    for (uint32_t i = 0; i < hclen; i++) {
        if (!in.take(3, v)) return "truncated input";
        cl[order[i]] = (uint8_t)v;
    }
    int rc = build_table(cl, 19, kCodesRoot, true, T.codes, 1 << kCodesRoot);
    if (rc) return rc == kHuffOver ? "over-subscribed code-length code" : "incomplete code-length code";
    const uint32_t total = hlit + hdist;
    for (uint32_t i = 0; i < total;) {
        in.refill();
        uint32_t sym;
        if (const char *why = decode_symbol(in, T.codes, kCodesRoot, sym)) return why;
        if (sym < 16) { lens[i++] = (uint8_t)sym; continue; }
        uint32_t rep;
        uint8_t fill = 0;
        if (sym == 16) {
            if (i == 0) return "a code-length repeat with no previous length";
            fill = lens[i - 1];
            if (take_extra(in, 2, rep)) return "truncated input";
            rep += 3;
        } else if (sym == 17) {
            if (take_extra(in, 3, rep)) return "truncated input";
            rep += 3;
        } else {
            if (take_extra(in, 7, rep)) return "truncated input";
            rep += 11;
        }
        if (i + rep > total) return "a code-length repeat past HLIT + HDIST";
        while (rep--) lens[i++] = fill;
    }
    if (!lens[256]) return "no end-of-block code";
    rc = build_table(lens, (int)hlit, kLitRoot, false, T.lit, kLitTable);
    if (rc) return rc == kHuffOver ? "over-subscribed literal/length code" : "incomplete literal/length code";
    rc = build_table(lens + hlit, (int)hdist, kDistRoot, false, T.dist, kDistTable);
    if (rc) return rc == kHuffOver ? "over-subscribed distance code" : "incomplete distance code";
    return nullptr;
}

void fixed_tables(InflateTables &T)
{
    uint8_t lens[288];
    for (int i = 0; i < 288; i++) lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
    build_table(lens, 288, kLitRoot, false, T.lit, kLitTable);
    memset(lens, 5, 32);
    build_table(lens, 32, kDistRoot, false, T.dist, kDistTable);
}

// The zlib stream -> exactly `want` bytes; 0, or what is wrong with it
const char *inflate_stream(BitIn &in, uint8_t *out, size_t want, InflateTables &T)
{
    static const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    static const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    uint32_t cmf, flg;
    if (!in.take(8, cmf) || !in.take(8, flg)) return "truncated input";
    if ((cmf & 15) != 8) return "zlib header: the method is not deflate";
    if ((cmf >> 4) > 7) return "zlib header: a window above 32 K";
    if ((cmf * 256 + flg) % 31) return "zlib header: FCHECK";
    if (flg & 0x20) return "zlib header: a preset dictionary";
    size_t o = 0;
    for (;;) {
        uint32_t last, type;
        if (!in.take(1, last) || !in.take(2, type)) return "truncated input";
        if (type == 3) return "block type 3";
        if (type == 0) {
            uint32_t len, nlen;
            in.align();
            if (!in.take(16, len) || !in.take(16, nlen)) return "truncated input";
            if ((len ^ 0xffffu) != nlen) return "stored block: LEN is not the complement of NLEN";
            if (len > want - o) return "the stream holds more than the image's bytes";
            if (!in.read_bytes(out + o, len)) return "truncated input";
            o += len;
        } else {
            if (type == 1) fixed_tables(T);
            else if (const char *why = read_dynamic(in, T)) return why;
            for (;;) {
                in.refill();
                uint32_t sym, extra;
                if (const char *why = decode_symbol(in, T.lit, kLitRoot, sym)) return why;
                if (sym < 256) {
                    if (o >= want) return "the stream holds more than the image's bytes";
                    out[o++] = (uint8_t)sym;
                    continue;
                }
                if (sym == 256) break;
                sym -= 257;
                if (sym >= 29) return "a length code above 285";
                if (const char *why = take_extra(in, lext[sym], extra)) return why;
                const size_t len = lbase[sym] + extra;
                if (const char *why = decode_symbol(in, T.dist, kDistRoot, sym)) return why;
                if (sym >= 30) return "a distance code above 29";
                if (const char *why = take_extra(in, dext[sym], extra)) return why;
                const size_t dist = dbase[sym] + extra;
                if (dist > o) return "a distance before the start of the output";
                if (len > want - o) return "the stream holds more than the image's bytes";
                uint8_t *to = out + o;
                const uint8_t *from = to - dist;
                if (dist >= len) memcpy(to, from, len);
                else for (size_t k = 0; k < len; k++) to[k] = from[k];
                o += len;
            }
        }
        if (last) break;
    }
    if (o != want) return "the stream holds fewer than the image's bytes";
    in.align();
    uint32_t sum = 0, v;
    for (int k = 0; k < 4; k++) {
        if (!in.take(8, v)) return "truncated input";
        sum = sum << 8 | v;
    }
    if (sum != adler32(out, want)) return "wrong Adler-32";
    return nullptr;
}

int png_inflate(const uint8_t *data, size_t size, const sv_png_info *info, uint8_t *filtered, size_t cap, uint8_t *row_filter)
{
    if (!data || !filtered) return sv_fail(SV_ERR_BAD_ARG, "sv_png_inflate: NULL argument");
    if (!sv_png_geometry_ok(info) || info->palette_entries < 0 || info->palette_entries > 256 || info->idat_offset < 8)
        return sv_fail(SV_ERR_BAD_ARG, "sv_png_inflate: the info was not made by sv_png_parse");
    const size_t want = (size_t)info->filtered_bytes;
    if (cap < want) return sv_fail(SV_ERR_BUFFER, "sv_png_inflate: the image takes %zu filtered bytes, the buffer holds %zu", want, cap);
    auto tables = std::make_unique<InflateTables>();
    BitIn in(data, size, (size_t)info->idat_offset);
    if (const char *why = inflate_stream(in, filtered, want, *tables)) return sv_fail(SV_ERR_BAD_ARG, "sv_png_inflate: %s", why);
    const size_t row = 1 + (size_t)info->row_bytes;
    for (long r = 0; r < info->height; r++) {
        const uint8_t f = filtered[(size_t)r * row];
        if (f > 4) return sv_fail(SV_ERR_BAD_ARG, "sv_png_inflate: row %ld has filter type %d", r, f);
        if (row_filter) row_filter[r] = f;
    }
    return SV_OK;
}

}  // namespace

// The one statement of which geometries exist: IHDR's five fields inside the decoder's limits, and the derived fields what png_derive makes of them
bool sv_png_geometry_ok(const sv_png_info *info)
{
    if (!info || info->width <= 0 || info->height <= 0 || info->width > SV_PNG_MAX_SIDE || info->height > SV_PNG_MAX_SIDE || info->interlace != 0 ||
        !png_channels(info->color_type) || !png_depth_ok(info->color_type, info->bit_depth))
        return false;
    sv_png_info want = *info;
    png_derive(&want);
    return want.channels == info->channels && want.bpp == info->bpp && want.row_bytes == info->row_bytes && want.filtered_bytes == info->filtered_bytes &&
           info->filtered_bytes <= SV_PNG_MAX_FILTERED_BYTES;
}

extern "C" int sv_png_parse(const uint8_t *d, size_t size, sv_png_info *info)
{
    if (!d || !info) return sv_fail(SV_ERR_BAD_ARG, "sv_png_parse: NULL argument");
    memset(info, 0, sizeof *info);
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (size < 8 || memcmp(d, sig, 8) != 0) return sv_fail(SV_ERR_BAD_ARG, "sv_png_parse: not a PNG signature");
    size_t at = 8;
    bool ihdr = false, plte = false, idat = false, idat_over = false, iend = false;
    const char *unsupported = nullptr;
    while (!iend) {
        if (size - at < 12) return sv_fail(SV_ERR_BAD_ARG, "sv_png_parse: the file ends before IEND");
        const uint32_t len = rd32(d + at);
        if (len > 0x7fffffffu || len > size - at - 12) return sv_fail(SV_ERR_BAD_ARG, "sv_png_parse: a chunk of %u bytes at offset %zu runs past the file", len, at);
        const uint8_t *type = d + at + 4, *body = d + at + 8;
        const bool critical = !(type[0] & 0x20);
        if (critical && crc32_update(0, type, 4 + (size_t)len) != rd32(body + len))
            return sv_fail(SV_ERR_BAD_ARG, "sv_png_parse: chunk %.4s at offset %zu: wrong CRC", (const char *)type, at);
        const bool is_idat = memcmp(type, "IDAT", 4) == 0;
        if (!ihdr && memcmp(type, "IHDR", 4) != 0) return sv_fail(SV_ERR_BAD_ARG, "sv_png_parse: the first chunk is not IHDR");
        if (memcmp(type, "IHDR", 4) == 0) {
            if (ihdr || len != 13) return sv_fail(SV_ERR_BAD_ARG, "sv_png_parse: a second or malformed IHDR");
            ihdr = true;
            const uint32_t w = rd32(body), h = rd32(body + 4);
            if (w == 0 || h == 0 || w > 0x7fffffffu || h > 0x7fffffffu) return sv_fail(SV_ERR_BAD_ARG, "sv_png_parse: size %u x %u", w, h);
            info->bit_depth = body[8]; info->color_type = body[9]; info->interlace = body[12];
            if (!png_channels(info->color_type) || !png_depth_ok(info->color_type, info->bit_depth))
                return sv_fail(SV_ERR_BAD_ARG, "sv_png_parse: colour type %d at %d bits is not in the specification", info->color_type, info->bit_depth);
            if (body[10] != 0 || body[11] != 0 || body[12] > 1) return sv_fail(SV_ERR_BAD_ARG, "sv_png_parse: unknown compression, filter or interlace method");
            if (body[12] == 1) unsupported = "an Adam7 interlaced file";
            if (w > SV_PNG_MAX_SIDE || h > SV_PNG_MAX_SIDE) unsupported = "a side above 65,535";
            else {
                info->width = (int)w; info->height = (int)h;
                png_derive(info);
                if (info->filtered_bytes > SV_PNG_MAX_FILTERED_BYTES) unsupported = "more than 512 MiB of filtered bytes";
            }
        } else if (memcmp(type, "PLTE", 4) == 0) {
            if (plte || idat || len == 0 || len % 3 || len > 768) return sv_fail(SV_ERR_BAD_ARG, "sv_png_parse: a second, late or malformed PLTE");
            plte = true;
            info->palette_entries = (int)(len / 3);
            memcpy(info->palette, body, len);
        } else if (is_idat) {
            if (idat_over) return sv_fail(SV_ERR_BAD_ARG, "sv_png_parse: IDAT chunks are not consecutive");
            if (!idat) info->idat_offset = (long)at;
            idat = true;
        } else if (memcmp(type, "IEND", 4) == 0) {
            iend = true;
        } else if (critical) {
            return sv_fail(SV_ERR_BAD_ARG, "sv_png_parse: unknown critical chunk %.4s", (const char *)type);
        }
        if (idat && !is_idat) idat_over = true;
        at += 12 + (size_t)len;
    }
    if (!idat) return sv_fail(SV_ERR_BAD_ARG, "sv_png_parse: no IDAT chunk");
    if (info->color_type == 3 && !plte) return sv_fail(SV_ERR_BAD_ARG, "sv_png_parse: colour type 3 without PLTE");
    if (unsupported) return sv_fail(SV_ERR_UNSUPPORTED, "sv_png_parse: %s is not decoded", unsupported);
    return SV_OK;
}

extern "C" int sv_png_inflate(const uint8_t *data, size_t size, const sv_png_info *info, uint8_t *filtered, size_t cap, uint8_t *row_filter)
{
    return png_inflate(data, size, info, filtered, cap, row_filter);
}

extern "C" int sv_png_inflate_batch(const uint8_t *const *datas, const size_t *sizes, const sv_png_info *infos, int n, uint8_t *const *filtered, const size_t *caps,
                                    uint8_t *const *row_filters, int threads, int *status)
{
    if (!datas || !sizes || !infos || !filtered || !caps || !status || n <= 0) return sv_fail(SV_ERR_BAD_ARG, "sv_png_inflate_batch: bad argument");
    auto one = [&](int i) { status[i] = png_inflate(datas[i], sizes[i], infos + i, filtered[i], caps[i], row_filters ? row_filters[i] : nullptr); };
    WorkerPool::instance().parallel_for(n, threads < 1 ? 1 : threads, one);
    for (int i = 0; i < n; i++)
        if (status[i] != SV_OK) return sv_fail(status[i], "sv_png_inflate_batch: image %d failed (see status[])", i);
    return SV_OK;
}
