// Host half of the JPEG front end (scope row N4: what cv2.imread does at pipeline/run.py:250 before the hot path starts).
// A baseline JPEG is a serial Huffman bit stream -- that part stays on the CPU, as the corner search does -- followed by
// per-block arithmetic (dequantise, inverse DCT, chroma interpolation, colour conversion) that is embarrassingly parallel
// and runs on the GPU (k5_jpeg.hip).  This file: marker parsing (SOF0/SOF1, DQT, DHT, DRI, SOS, JFIF/Adobe/EXIF) and entropy
// decoding into dense int16 coefficient blocks, natural (de-zigzagged) order, laid out per component over the MCU-padded
// block grid -- the layout the reconstruction kernels index directly.
//
// Speed: a 64-bit bit buffer refilled a byte at a time only around 0xFF, a 10-bit look-ahead table per Huffman table that
// resolves (code length, symbol) in one probe, restart intervals located up front by a memchr scan and decoded in parallel
// (each interval is an independent bit stream with its own DC predictors), images of a batch spread over the same pool.
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sv_internal.h"
#include "host_pool.h"

namespace {

constexpr int kLook = 10;

const uint8_t kNatural[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                              35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffTable {
    uint16_t look[1 << kLook];          // (length << 8) | symbol for codes of <= kLook bits, 0 otherwise
    int32_t maxcode[18];                // per length, left-aligned to 16 bits (exclusive upper bound); sentinel at [17]
    int32_t delta[17];                  // vals index = delta[len] + code
    uint8_t vals[256];
    int32_t fast_ac[1 << kLook];        // AC tables: (value << 16) | (run << 8) | total bits when code + magnitude bits fit kLook, else 0
    bool defined = false;

    bool define(const uint8_t *counts /*16*/, const uint8_t *symbols, int total)
    {
        memcpy(vals, symbols, (size_t)total);
        memset(look, 0, sizeof look);
        int code = 0, k = 0;
        for (int len = 1; len <= 16; len++) {
            delta[len] = k - code;
            if (code + counts[len - 1] > (1 << len)) return false;  // over-subscribed table: reject before look[] is indexed with its codes
            for (int i = 0; i < counts[len - 1]; i++, k++, code++) {
                if (len <= kLook) {
                    const int first = code << (kLook - len), span = 1 << (kLook - len);
                    for (int j = 0; j < span; j++) look[first + j] = (uint16_t)((len << 8) | vals[k]);
                }
            }
            maxcode[len] = code << (16 - len);
            code <<= 1;
        }
        maxcode[17] = 0x7fffffff;
        // short code + short magnitude in one probe: the bits after the code ARE the magnitude field
        for (int i = 0; i < (1 << kLook); i++) {
            fast_ac[i] = 0;
            const int e = look[i];
            if (!e) continue;
            const int len = e >> 8, run = (e >> 4) & 15, size = e & 15;
            if (size == 0 || len + size > kLook) continue;
            int v = (i >> (kLook - len - size)) & ((1 << size) - 1);
            if (v < (1 << (size - 1))) v += 1 - (1 << size);
            fast_ac[i] = (int32_t)((unsigned)v << 16 | (unsigned)run << 8 | (unsigned)(len + size));
        }
        defined = true;
        return true;
    }
};

struct Component { int id, h, v, tq, bw, bh; long offset; };

struct Header {
    int width = 0, height = 0, ncomp = 0, hmax = 1, vmax = 1, mcu_cols = 0, mcu_rows = 0;
    int restart_interval = 0, orientation = 1;
    bool jfif = false, adobe = false;
    int adobe_transform = 0;
    Component comp[3];
    uint16_t quant[4][64];
    bool quant_defined[4] = {false, false, false, false};
    HuffTable dc[4], ac[4];
    long coef_count = 0;
    long luma_count = 0;                                           // coefficients of component 0 alone
    size_t first_scan = 0;                                         // offset of the first SOS marker
};

inline unsigned be16(const uint8_t *p) { return (unsigned)p[0] << 8 | p[1]; }

// EXIF orientation tag (0x0112) of IFD0; cv2.imread rotates/flips accordingly
int exif_orientation(const uint8_t *seg, int n)
{
    if (n < 14 || memcmp(seg, "Exif\0\0", 6) != 0) return 1;
    const uint8_t *t = seg + 6;
    n -= 6;
    const bool little = t[0] == 'I' && t[1] == 'I';
    if (!little && !(t[0] == 'M' && t[1] == 'M')) return 1;
    auto u16 = [&](unsigned o) -> unsigned { return little ? (t[o] | t[o + 1] << 8) : (t[o] << 8 | t[o + 1]); };
    auto u32 = [&](unsigned o) -> unsigned { return little ? (u16(o) | u16(o + 2) << 16) : (u16(o) << 16 | u16(o + 2)); };
    if (u16(2) != 42) return 1;
    const unsigned ifd = u32(4);
    if (ifd > (unsigned)n || ifd + 2 > (unsigned)n) return 1;
    const unsigned entries = u16(ifd);
    for (unsigned i = 0; i < entries; i++) {
        const unsigned e = ifd + 2 + 12 * i;
        if (e + 12 > (unsigned)n) break;
        if (u16(e) == 0x0112) {
            const unsigned v = u16(e + 8);
            return v >= 1 && v <= 8 ? (int)v : 1;
        }
    }
    return 1;
}

// Table-definition segments can appear before any scan, so both the header pass and the scan loop use these
int read_dht(Header &h, const uint8_t *s, int n)
{
    while (n >= 17) {
        const int cls = s[0] >> 4, id = s[0] & 15;
        int total = 0;
        for (int i = 0; i < 16; i++) total += s[1 + i];
        if (cls > 1 || id > 3 || total > 256 || n < 17 + total) return sv_fail(SV_ERR_BAD_ARG, "jpeg: bad DHT segment");
        if (!(cls ? h.ac[id] : h.dc[id]).define(s + 1, s + 17, total)) return sv_fail(SV_ERR_BAD_ARG, "jpeg: over-subscribed Huffman table");
        s += 17 + total;
        n -= 17 + total;
    }
    return SV_OK;
}

int read_dqt(Header &h, const uint8_t *s, int n)
{
    while (n >= 65) {
        const int wide = s[0] >> 4, id = s[0] & 15;
        if (id > 3 || (wide && n < 129)) return sv_fail(SV_ERR_BAD_ARG, "jpeg: bad DQT segment");
        for (int i = 0; i < 64; i++) h.quant[id][kNatural[i]] = wide ? (uint16_t)be16(s + 1 + 2 * i) : s[1 + i];
        h.quant_defined[id] = true;
        s += wide ? 129 : 65;
        n -= wide ? 129 : 65;
    }
    return SV_OK;
}

// Walks marker segments from `pos`; returns the marker code and sets seg/len to its payload, or -1 at the end of data
int next_segment(const uint8_t *d, size_t size, size_t &pos, const uint8_t *&seg, int &len)
{
    for (;;) {
        const uint8_t *ff = pos < size ? (const uint8_t *)memchr(d + pos, 0xFF, size - pos) : nullptr;
        if (!ff) return -1;
        pos = (size_t)(ff - d);
        while (pos < size && d[pos] == 0xFF) pos++;
        if (pos >= size) return -1;
        const int m = d[pos++];
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD8)) continue;       // stuffing, TEM, RSTn, SOI: no payload
        if (m == 0xD9) { seg = nullptr; len = 0; return m; }
        if (pos + 2 > size) return -1;
        const int L = (int)be16(d + pos);
        if (L < 2 || pos + (size_t)L > size) return -1;
        seg = d + pos + 2;
        len = L - 2;
        pos += (size_t)L;
        return m;
    }
}

int parse_header(const uint8_t *d, size_t size, Header &h)
{
    if (!d || size < 4 || d[0] != 0xFF || d[1] != 0xD8) return sv_fail(SV_ERR_BAD_ARG, "jpeg: no SOI marker (not a JPEG file)");
    size_t pos = 2;
    bool have_frame = false;
    for (;;) {
        const uint8_t *s;
        int n;
        const size_t at = pos;
        const int m = next_segment(d, size, pos, s, n);
        if (m < 0 || m == 0xD9) return sv_fail(SV_ERR_BAD_ARG, "jpeg: no scan found");
        int rc = SV_OK;
        switch (m) {
        case 0xC0: case 0xC1: {
            if (n < 6) return sv_fail(SV_ERR_BAD_ARG, "jpeg: short SOF segment");
            if (s[0] != 8) return sv_fail(SV_ERR_UNSUPPORTED, "jpeg: %d-bit samples (only 8-bit is supported)", s[0]);
            h.height = (int)be16(s + 1); h.width = (int)be16(s + 3); h.ncomp = s[5];
            if (h.height == 0 || h.width == 0) return sv_fail(SV_ERR_UNSUPPORTED, "jpeg: image size deferred to a DNL marker");
            if (h.ncomp != 1 && h.ncomp != 3) return sv_fail(SV_ERR_UNSUPPORTED, "jpeg: %d components (gray or YCbCr only)", h.ncomp);
            if (n < 6 + 3 * h.ncomp) return sv_fail(SV_ERR_BAD_ARG, "jpeg: short SOF segment");
            for (int c = 0; c < h.ncomp; c++) h.comp[c] = {s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c] & 3, 0, 0, 0};
            have_frame = true;
            break;
        }
        case 0xC2: return sv_fail(SV_ERR_UNSUPPORTED, "jpeg: progressive files are not supported (baseline / extended sequential Huffman only)");
        case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF:
            return sv_fail(SV_ERR_UNSUPPORTED, "jpeg: SOF%d (lossless / hierarchical / arithmetic) is not supported", m - 0xC0);
        case 0xC4: rc = read_dht(h, s, n); break;
        case 0xDB: rc = read_dqt(h, s, n); break;
        case 0xDD: if (n < 2) return sv_fail(SV_ERR_BAD_ARG, "jpeg: short DRI segment"); h.restart_interval = (int)be16(s); break;
        case 0xE0: if (n >= 5 && memcmp(s, "JFIF", 5) == 0) h.jfif = true; break;
        case 0xE1: { const int o = exif_orientation(s, n); if (o != 1) h.orientation = o; break; }
        case 0xEE: if (n >= 12 && memcmp(s, "Adobe", 5) == 0) { h.adobe = true; h.adobe_transform = s[11]; } break;
        case 0xDA: h.first_scan = at; goto scanned;
        default: break;
        }
        if (rc) return rc;
    }
scanned:
    if (!have_frame) return sv_fail(SV_ERR_BAD_ARG, "jpeg: scan before frame header");
    if (h.ncomp == 1) h.comp[0].h = h.comp[0].v = 1;
    else {
        const Component *c = h.comp;
        const bool chroma_full = c[1].h == 1 && c[1].v == 1 && c[2].h == 1 && c[2].v == 1;
        const bool luma_ok = (c[0].h == 1 && c[0].v == 1) || (c[0].h == 2 && (c[0].v == 1 || c[0].v == 2));
        if (!chroma_full || !luma_ok)
            return sv_fail(SV_ERR_UNSUPPORTED, "jpeg: sampling %dx%d,%dx%d,%dx%d (4:4:4, 4:2:2 and 4:2:0 are supported)", c[0].h, c[0].v, c[1].h, c[1].v, c[2].h, c[2].v);
        if ((h.adobe && h.adobe_transform != 1) || (!h.jfif && !h.adobe && c[0].id == 'R' && c[1].id == 'G' && c[2].id == 'B'))
            return sv_fail(SV_ERR_UNSUPPORTED, "jpeg: not a YCbCr file");
    }
    h.hmax = h.comp[0].h;
    h.vmax = h.comp[0].v;
    h.mcu_cols = (h.width + 8 * h.hmax - 1) / (8 * h.hmax);
    h.mcu_rows = (h.height + 8 * h.vmax - 1) / (8 * h.vmax);
    long off = 0;
    for (int c = 0; c < h.ncomp; c++) {
        h.comp[c].bw = h.mcu_cols * h.comp[c].h;
        h.comp[c].bh = h.mcu_rows * h.comp[c].v;
        h.comp[c].offset = off;
        off += (long)h.comp[c].bw * h.comp[c].bh * 64;
    }
    h.coef_count = off;
    h.luma_count = (long)h.comp[0].bw * h.comp[0].bh * 64;
    return SV_OK;
}

long sparse_capacity(const Header &h, size_t size, bool luma);

// luma: the counts of the luma-only decode (Y's blocks alone) in place of the file's
void export_info(const Header &h, size_t size, sv_jpeg_info *o, bool luma = false)
{
    o->sparse_capacity = sparse_capacity(h, size, luma);
    const bool swap = h.orientation >= 5;
    o->width = h.width; o->height = h.height;
    o->out_width = swap ? h.height : h.width; o->out_height = swap ? h.width : h.height;
    o->components = h.ncomp; o->h_samp = h.hmax; o->v_samp = h.vmax;
    o->orientation = h.orientation; o->restart_interval = h.restart_interval;
    o->coef_count = luma ? h.luma_count : h.coef_count;
}

// ---- the bit stream of one restart interval ----------------------------------------------------------
struct BitStream {
    const uint8_t *p, *end;
    uint64_t acc = 0;                   // bits left-aligned
    int have = 0;
    long fake = 0;                      // zero bits appended after the interval's last byte (they sit at the tail of the buffer)

    BitStream(const uint8_t *b, const uint8_t *e) : p(b), end(e) {}

    inline void refill()                // afterwards at least 32 bits are buffered (code <= 16 + magnitude <= 16)
    {
        if (have > 32) return;
        if (p + 4 <= end) {             // four bytes at once when none of them is 0xFF (the common case)
            const uint32_t w = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
            if (((~w - 0x01010101u) & w & 0x80808080u) == 0) {
                acc |= (uint64_t)w << (32 - have);
                have += 32;
                p += 4;
                return;
            }
        }
        while (have <= 56) {
            unsigned c = 0;
            if (p < end) {
                c = *p++;
                if (c == 0xFF && p < end && *p == 0x00) p++;        // byte stuffing; the interval ends before any real marker
            }
            else fake += 8;
            acc |= (uint64_t)c << (56 - have);
            have += 8;
        }
    }
    // true once decoding has consumed bits that are not in the file (a truncated or corrupt interval)
    inline bool starved() const { return (long)have < fake; }
    inline unsigned peek16() const { return (unsigned)(acc >> 48); }
    inline void drop(int n) { acc <<= n; have -= n; }
    inline int take_signed(int s)       // RECEIVE + EXTEND (T.81 F.2.2.1)
    {
        const int v = (int)(acc >> (64 - s));
        drop(s);
        return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
    }
    inline int symbol(const HuffTable &t)
    {
        const unsigned top = peek16();
        const unsigned e = t.look[top >> (16 - kLook)];
        if (e) { drop((int)(e >> 8)); return (int)(e & 255); }
        int len = kLook + 1;
        while ((int)top >= t.maxcode[len]) len++;
        if (len > 16) { drop(16); return 0; }                      // invalid code: libjpeg substitutes 0 and goes on
        drop(len);
        return t.vals[(t.delta[len] + (int)(top >> (16 - len))) & 255];
    }
};

struct ScanComponent { int comp, dc, ac, nh, nv; };

struct Scan {
    int ns = 0;
    ScanComponent sc[3];
    int mcu_cols = 0, mcu_rows = 0;
};

// Where decoded blocks go.  Dense: 64 int16 per block, natural order.  Sparse (the PCIe transport): per block a 64-bit
// mask over ZIGZAG positions and the index of its first value; the non-zero values themselves are appended, in zigzag order,
// to a value stream -- a q90 1080p frame is ~0.6 M values + 12 B per block instead of 3.1 M int16.
struct DenseOut { int16_t *coef; };
struct SparseOut { uint64_t *masks; uint32_t *offs; int16_t *vals; };

// Decodes MCUs [m0, m1) of a scan from one restart interval's bytes.  Sparse: values are appended from index `vpos` on, never
// at or beyond `vlimit`; returns the index after the last value written (dense: 0).
// Insufficient data, as libjpeg handles it (jdhuff.c: insufficient_data, reset at every restart): once decoding needs bits the
// interval does not hold, the block being decoded and every later block of the interval stay zero (they reconstruct as mid-grey),
// which is what cv2.imread / Pillow(LOAD_TRUNCATED_IMAGES) show for the tail of a cut file.
// LUMA: the output holds component 0 alone, in scan order -- MCU after MCU, an MCU's h x v blocks row-major -- so that a block's raster position
// follows from its index (k20_jpeg_gray.hip: luma_record).  The other components' blocks are parsed, as they must be to stay in step with the bit
// stream and the DC predictors, and stored nowhere.
template <bool SPARSE, bool LUMA, class Out>
long decode_interval(const Header &h, const Scan &scan, const uint8_t *b, const uint8_t *e, long m0, long m1, const Out &out, long vpos, long vlimit)
{
    BitStream bs(b, e);
    int pred[3] = {0, 0, 0};
    bool dead = false;
    for (long mi = m0; mi < m1; mi++) {
        const int mx = (int)(mi % scan.mcu_cols), my = (int)(mi / scan.mcu_cols);
        for (int i = 0; i < scan.ns; i++) {
            const ScanComponent &s = scan.sc[i];
            const Component &c = h.comp[s.comp];
            const HuffTable &dct = h.dc[s.dc], &act = h.ac[s.ac];
            const bool keep = !LUMA || s.comp == 0;
            for (int v = 0; v < s.nv; v++)
                for (int u = 0; u < s.nh; u++) {
                    const int bx = mx * s.nh + u, by = my * s.nv + v;
                    const long bi = LUMA ? ((long)(by / c.v) * h.mcu_cols + bx / c.h) * (c.h * c.v) + (by % c.v) * c.h + bx % c.h
                                         : c.offset / 64 + (long)by * c.bw + bx;
                    int16_t skipped[64];                            // LUMA: where a block of another component is decoded to
                    int16_t *blk = nullptr;
                    uint64_t mask = 0;
                    const long vstart = vpos;
                    if constexpr (!SPARSE) {
                        blk = keep ? out.coef + bi * 64 : skipped;
                        if (keep) memset(blk, 0, 64 * sizeof(int16_t));      // cleared while the lines are about to be written anyway
                    }
                    if (dead) {
                        if constexpr (SPARSE) { if (keep) { out.masks[bi] = 0; out.offs[bi] = (uint32_t)vstart; } }
                        continue;
                    }
                    bool full = false;                              // sparse: the interval's stretch of the value stream is used up
                    bs.refill();
                    const int t = bs.symbol(dct) & 15;
                    if (t) pred[i] += bs.take_signed(t);
                    if constexpr (SPARSE) {
                        if ((int16_t)pred[i] && keep) {
                            if (vpos < vlimit) { mask = 1; out.vals[vpos++] = (int16_t)pred[i]; } else full = true;
                        }
                    } else blk[0] = (int16_t)pred[i];
                    for (int k = 1; k < 64 && !full;) {
                        bs.refill();
                        const int32_t f = act.fast_ac[bs.peek16() >> (16 - kLook)];
                        int val;
                        if (f) {
                            k += (f >> 8) & 15;
                            if (k > 63) break;
                            bs.drop(f & 255);
                            val = f >> 16;
                        } else {
                            const int rs = bs.symbol(act), run = rs >> 4, size = rs & 15;
                            if (size == 0) {
                                if (run != 15) break;               // EOB
                                k += 16;
                                continue;
                            }
                            k += run;
                            if (k > 63) break;
                            val = bs.take_signed(size);
                        }
                        if constexpr (SPARSE) {
                            if ((int16_t)val && keep) {
                                if (vpos < vlimit) { mask |= 1ull << k; out.vals[vpos++] = (int16_t)val; } else full = true;
                            }
                        } else blk[kNatural[k]] = (int16_t)val;
                        k++;
                    }
                    if (bs.starved() || full) {                     // this block was (partly) made of bits that are not there: drop it and the rest
                        dead = true;
                        mask = 0;
                        vpos = vstart;
                        if constexpr (!SPARSE) { if (keep) memset(blk, 0, 64 * sizeof(int16_t)); }
                    }
                    if constexpr (SPARSE) { if (keep) { out.masks[bi] = mask; out.offs[bi] = (uint32_t)vstart; } }
                }
        }
    }
    return vpos;
}

// every non-zero value costs at least 2 bits (code >= 1, magnitude >= 1): an interval of n bytes holds at most 4n values
inline long interval_value_bound(size_t bytes) { return 4 * (long)bytes + 2; }

// Splits the entropy-coded bytes that start at `pos` into restart intervals; returns the offset of the marker that ends the scan
size_t split_intervals(const uint8_t *d, size_t size, size_t pos, std::vector<std::pair<size_t, size_t>> &out)
{
    size_t start = pos;
    for (;;) {
        const uint8_t *ff = pos < size ? (const uint8_t *)memchr(d + pos, 0xFF, size - pos) : nullptr;
        if (!ff || (size_t)(ff - d) + 1 >= size) { out.emplace_back(start, size); return size; }
        const size_t at = (size_t)(ff - d);
        const int m = d[at + 1];
        if (m == 0x00) { pos = at + 2; continue; }
        if (m == 0xFF) { pos = at + 1; continue; }
        if (m >= 0xD0 && m <= 0xD7) { out.emplace_back(start, at); start = pos = at + 2; continue; }
        out.emplace_back(start, at);
        return at;
    }
}

template <bool SPARSE, bool LUMA, class Out>
int entropy_decode(const uint8_t *d, size_t size, Header &h, const Out &out, int threads, long vals_cap, long *vals_used)
{
    bool first = true;
    size_t pos = h.first_scan;
    unsigned covered = 0;                                          // bit c: component c has been decoded
    const unsigned all = (1u << h.ncomp) - 1;
    long vbase = 0;                                                // sparse: where the next scan's value regions start
    while (covered != all) {
        const uint8_t *s;
        int n;
        const int m = next_segment(d, size, pos, s, n);
        if (m < 0 || m == 0xD9) return sv_fail(SV_ERR_BAD_ARG, "jpeg: data ends before all components were decoded");
        if (m == 0xC4) { const int rc = read_dht(h, s, n); if (rc) return rc; continue; }
        if (m == 0xDD) { if (n < 2) return sv_fail(SV_ERR_BAD_ARG, "jpeg: short DRI segment"); h.restart_interval = (int)be16(s); continue; }
        if (m != 0xDA) continue;
        Scan scan;
        scan.ns = n >= 1 ? s[0] : 0;
        if (scan.ns < 1 || scan.ns > h.ncomp || n < 4 + 2 * scan.ns) return sv_fail(SV_ERR_BAD_ARG, "jpeg: bad SOS segment");
        for (int i = 0; i < scan.ns; i++) {
            int c = 0;
            while (c < h.ncomp && h.comp[c].id != s[1 + 2 * i]) c++;
            const int td = s[2 + 2 * i] >> 4, ta = s[2 + 2 * i] & 15;
            if (c == h.ncomp || td > 3 || ta > 3 || !h.dc[td].defined || !h.ac[ta].defined) return sv_fail(SV_ERR_BAD_ARG, "jpeg: scan refers to an undefined component or table");
            if (covered >> c & 1) return sv_fail(SV_ERR_BAD_ARG, "jpeg: component %d appears in more than one scan (or twice in one)", c);
            covered |= 1u << c;
            scan.sc[i] = {c, td, ta, scan.ns == 1 ? 1 : h.comp[c].h, scan.ns == 1 ? 1 : h.comp[c].v};
        }
        const uint8_t *tail = s + 1 + 2 * scan.ns;
        if (tail[0] != 0 || tail[1] != 63 || tail[2] != 0) return sv_fail(SV_ERR_UNSUPPORTED, "jpeg: spectral selection / successive approximation in a sequential file");
        if (first && scan.ns < h.ncomp) {                          // only a full interleave reaches (and clears) every block: a
            const long count = LUMA ? h.luma_count : h.coef_count; // component's own block grid leaves the MCU padding blocks out
            if constexpr (SPARSE) {
                memset(out.masks, 0, (size_t)(count / 64) * sizeof(uint64_t));
                memset(out.offs, 0, (size_t)(count / 64) * sizeof(uint32_t));
            } else memset(out.coef, 0, (size_t)count * sizeof(int16_t));
        }
        first = false;
        if (scan.ns == 1) {                                        // non-interleaved: the component's own block grid
            const Component &c = h.comp[scan.sc[0].comp];
            scan.mcu_cols = ((h.width * c.h + h.hmax - 1) / h.hmax + 7) / 8;
            scan.mcu_rows = ((h.height * c.v + h.vmax - 1) / h.vmax + 7) / 8;
        } else { scan.mcu_cols = h.mcu_cols; scan.mcu_rows = h.mcu_rows; }
        const long nmcu = (long)scan.mcu_cols * scan.mcu_rows;
        std::vector<std::pair<size_t, size_t>> iv;
        pos = split_intervals(d, size, pos, iv);
        const long per = h.restart_interval > 0 ? h.restart_interval : nmcu;
        const long need = (nmcu + per - 1) / per;
        if ((long)iv.size() < need) return sv_fail(SV_ERR_BAD_ARG, "jpeg: %ld restart intervals found, %ld needed (truncated file?)", (long)iv.size(), need);
        std::vector<long> vstart((size_t)need + 1, 0), vend((size_t)need, 0);
        if constexpr (SPARSE) {                                    // each interval appends to its own stretch of the value stream
            vstart[0] = vbase;
            for (long k = 0; k < need; k++) {
                long blocks = 0;
                for (int i = 0; i < scan.ns; i++)
                    if (!LUMA || scan.sc[i].comp == 0) blocks += (long)scan.sc[i].nh * scan.sc[i].nv;
                const long m0 = k * per, m1 = std::min(nmcu, m0 + per);
                vstart[k + 1] = vstart[k] + std::min(interval_value_bound(iv[k].second - iv[k].first), (m1 - m0) * blocks * 64);
            }
            if (vstart[need] > vals_cap) return sv_fail(SV_ERR_BUFFER, "jpeg: value buffer holds %ld, this file may need %ld", vals_cap, vstart[need]);
        }
        const Header &hc = h;
        WorkerPool::instance().parallel_for((int)need, threads, [&](int k) {
            const long m0 = (long)k * per, m1 = std::min(nmcu, m0 + per);
            vend[k] = decode_interval<SPARSE, LUMA>(hc, scan, d + iv[k].first, d + iv[k].second, m0, m1, out, vstart[k], SPARSE ? vstart[k + 1] : 0);
        });
        if constexpr (SPARSE) {
            vbase = vstart[need];
            if (vals_used) *vals_used = vend[need - 1];            // everything the kernels can reference lies below this index
        }
    }
    return SV_OK;
}

int fill_quant(const Header &h, uint16_t *quant)
{
    memset(quant, 0, 3 * 64 * sizeof(uint16_t));
    for (int c = 0; c < h.ncomp; c++) {
        if (!h.quant_defined[h.comp[c].tq]) return sv_fail(SV_ERR_BAD_ARG, "jpeg: component %d uses an undefined quantisation table", c);
        memcpy(quant + 64 * c, h.quant[h.comp[c].tq], 64 * sizeof(uint16_t));
    }
    return SV_OK;
}

long sparse_capacity(const Header &h, size_t size, bool luma)
{
    const long nmcu = (long)h.mcu_cols * h.mcu_rows;
    const long intervals = h.restart_interval > 0 ? (nmcu + h.restart_interval - 1) / h.restart_interval : 1;
    // a single-component file: the luma mode is the existing decode
    if (!luma || h.ncomp == 1) return std::min(h.coef_count, 4 * (long)size + 2 * 3 * intervals + 64);
    // Y's values lie in the one scan that holds Y; in a scan of its own an MCU is a single block, so there are at most this many intervals
    const long yint = h.restart_interval > 0 ? (h.luma_count / 64 + h.restart_interval - 1) / h.restart_interval : 1;
    return std::min(h.luma_count, 4 * (long)size + 2 * yint + 64);
}

// One file, start to end: the header, every component's quantiser steps, the scan loop.  LUMA: the steps of all three components are still
// looked up (a refusal of the full decode is a refusal here), quant receives Y's 64 alone.
template <bool SPARSE, bool LUMA, class Out>
int decode_file(const uint8_t *data, size_t size, Header &h, const Out &out, uint16_t *quant, int threads, long vals_cap, long *vals_used)
{
    uint16_t all[192];
    int rc = parse_header(data, size, h);
    if (rc || (rc = fill_quant(h, LUMA ? all : quant))) return rc;
    if (LUMA) memcpy(quant, all, 64 * sizeof(uint16_t));
    if (vals_used) *vals_used = 0;
    return entropy_decode<SPARSE, LUMA>(data, size, h, out, threads, vals_cap, vals_used);
}

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------
extern "C" int sv_jpeg_parse(const uint8_t *data, size_t size, sv_jpeg_info *info)
{
    if (!data || !info) return sv_fail(SV_ERR_BAD_ARG, "sv_jpeg_parse: NULL argument");
    std::unique_ptr<Header> h(new Header);
    const int rc = parse_header(data, size, *h);
    if (rc) return rc;
    export_info(*h, size, info);
    return SV_OK;
}

extern "C" int sv_jpeg_parse_luma(const uint8_t *data, size_t size, sv_jpeg_info *info)
{
    if (!data || !info) return sv_fail(SV_ERR_BAD_ARG, "sv_jpeg_parse_luma: NULL argument");
    std::unique_ptr<Header> h(new Header);
    const int rc = parse_header(data, size, *h);
    if (rc) return rc;
    export_info(*h, size, info, true);
    return SV_OK;
}

extern "C" int sv_jpeg_entropy_decode(const uint8_t *data, size_t size, int16_t *coef, uint16_t *quant, int threads)
{
    if (!data || !coef || !quant) return sv_fail(SV_ERR_BAD_ARG, "sv_jpeg_entropy_decode: NULL argument");
    std::unique_ptr<Header> h(new Header);
    return decode_file<false, false>(data, size, *h, DenseOut{coef}, quant, threads < 1 ? 1 : threads, 0, nullptr);
}

extern "C" int sv_jpeg_entropy_decode_luma(const uint8_t *data, size_t size, int16_t *coef, uint16_t *quant, int threads)
{
    if (!data || !coef || !quant) return sv_fail(SV_ERR_BAD_ARG, "sv_jpeg_entropy_decode_luma: NULL argument");
    std::unique_ptr<Header> h(new Header);
    return decode_file<false, true>(data, size, *h, DenseOut{coef}, quant, threads < 1 ? 1 : threads, 0, nullptr);
}

extern "C" int sv_jpeg_entropy_decode_sparse(const uint8_t *data, size_t size, uint64_t *masks, uint32_t *offsets, int16_t *values, long values_cap,
                                             long *values_used, uint16_t *quant, int threads)
{
    if (!data || !masks || !offsets || !values || !values_used || !quant) return sv_fail(SV_ERR_BAD_ARG, "sv_jpeg_entropy_decode_sparse: NULL argument");
    std::unique_ptr<Header> h(new Header);
    return decode_file<true, false>(data, size, *h, SparseOut{masks, offsets, values}, quant, threads < 1 ? 1 : threads, values_cap, values_used);
}

extern "C" int sv_jpeg_entropy_decode_luma_sparse(const uint8_t *data, size_t size, uint64_t *masks, uint32_t *offsets, int16_t *values, long values_cap,
                                                  long *values_used, uint16_t *quant, int threads)
{
    if (!data || !masks || !offsets || !values || !values_used || !quant) return sv_fail(SV_ERR_BAD_ARG, "sv_jpeg_entropy_decode_luma_sparse: NULL argument");
    std::unique_ptr<Header> h(new Header);
    return decode_file<true, true>(data, size, *h, SparseOut{masks, offsets, values}, quant, threads < 1 ? 1 : threads, values_cap, values_used);
}

// Images of a batch over the pool's threads; every image decodes its restart intervals serially (a worker's nested
// parallel_for runs inline).  Dense when `coefs` is given, sparse when masks/offsets/values are.  LUMA: image i's quantiser steps are 64, not 192.
template <bool LUMA>
static int entropy_decode_batch(const char *fn, const uint8_t *const *datas, const size_t *sizes, int n, int16_t *const *coefs, uint64_t *const *masks,
                                uint32_t *const *offsets, int16_t *const *values, const long *values_cap, long *values_used, uint16_t *quants, int threads, int *status)
{
    const bool sparse = coefs == nullptr;
    if (!datas || !sizes || !quants || !status || n <= 0 || (sparse && (!masks || !offsets || !values || !values_cap || !values_used)))
        return sv_fail(SV_ERR_BAD_ARG, "%s: bad argument", fn);
    if (threads < 1) threads = 1;
    std::vector<std::unique_ptr<Header>> hs((size_t)n);
    auto one = [&](int i, int inner_threads) {
        hs[i].reset(new Header);
        const bool ok = datas[i] && (sparse ? (masks[i] && offsets[i] && values[i]) : coefs[i] != nullptr);
        uint16_t *q = quants + (LUMA ? 64 : 192) * (size_t)i;
        if (!ok) status[i] = SV_ERR_BAD_ARG;
        else if (sparse)
            status[i] = decode_file<true, LUMA>(datas[i], sizes[i], *hs[i], SparseOut{masks[i], offsets[i], values[i]}, q, inner_threads, values_cap[i], values_used + i);
        else status[i] = decode_file<false, LUMA>(datas[i], sizes[i], *hs[i], DenseOut{coefs[i]}, q, inner_threads, 0, nullptr);
    };
    if (threads == 1 || n == 1) for (int i = 0; i < n; i++) one(i, n == 1 ? threads : 1);
    else WorkerPool::instance().parallel_for(n, threads, [&](int i) { one(i, 1); });
    for (int i = 0; i < n; i++)
        if (status[i] != SV_OK) return sv_fail(status[i], "%s: image %d failed (see status[])", fn, i);
    return SV_OK;
}

extern "C" int sv_jpeg_entropy_decode_batch(const uint8_t *const *datas, const size_t *sizes, int n, int16_t *const *coefs, uint64_t *const *masks,
                                            uint32_t *const *offsets, int16_t *const *values, const long *values_cap, long *values_used,
                                            uint16_t *quants, int threads, int *status)
{
    return entropy_decode_batch<false>("sv_jpeg_entropy_decode_batch", datas, sizes, n, coefs, masks, offsets, values, values_cap, values_used, quants, threads, status);
}

extern "C" int sv_jpeg_entropy_decode_luma_batch(const uint8_t *const *datas, const size_t *sizes, int n, int16_t *const *coefs, uint64_t *const *masks,
                                                 uint32_t *const *offsets, int16_t *const *values, const long *values_cap, long *values_used,
                                                 uint16_t *quants, int threads, int *status)
{
    return entropy_decode_batch<true>("sv_jpeg_entropy_decode_luma_batch", datas, sizes, n, coefs, masks, offsets, values, values_cap, values_used, quants, threads, status);
}

// ---- the encoder's host half (cv2.imwrite at pipeline/run.py:431) ----------------------------------------
// The device half (k17_jpeg_encode.hip) leaves a frame as the sparse records above; what remains is serial: the marker segments jcmarker.c
// writes, and the Huffman bit stream of jchuff.c with the Annex K tables -- DC differences, (run, size) symbols over the mask's set bits (the
// runs of zeros are the gaps between them: one count-trailing-zeros per coefficient, no pass over the 64 positions), ZRL, EOB, 0xFF stuffing,
// 1-bit padding at the end of every restart interval.  Restart intervals are independent bit streams: `threads` contiguous runs of them are
// packed in parallel and concatenated.
namespace {

// T.81 Annex K.3: code counts per length 1..16, then the symbols
const uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
    0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
    0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
    0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
    0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
    0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
// T.81 Annex K.1, natural order
const uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                               18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

struct EncCodes {
    uint32_t code[256];
    uint8_t len[256];                                              // 0: the table has no code for the symbol
    void define(const uint8_t *counts, const uint8_t *symbols)
    {
        memset(len, 0, sizeof len);
        memset(code, 0, sizeof code);
        uint32_t c = 0;
        int k = 0;
        for (int l = 1; l <= 16; l++) {
            for (int i = 0; i < counts[l - 1]; i++, k++, c++) { code[symbols[k]] = c; len[symbols[k]] = (uint8_t)l; }
            c <<= 1;
        }
    }
};

struct EncTables {
    EncCodes dc[2], ac[2];                                         // [0] luma, [1] chroma
    EncTables()
    {
        dc[0].define(kDcLumaBits, kDcVals); dc[1].define(kDcChromaBits, kDcVals);
        ac[0].define(kAcLumaBits, kAcLumaVals); ac[1].define(kAcChromaBits, kAcChromaVals);
    }
};
const EncTables &enc_tables() { static const EncTables t; return t; }

constexpr long kEncHeaderMax = 640;                                // SOI 2, APP0 18, DQT 2 x 69, SOF0 19, DHT 432, DRI 6, SOS 14, EOI 2 = 631
// A block costs at most 20 bits of DC, 3 ZRL of 11 bits and an EOB of 4; a non-zero AC value at most 16 + 10.  Twice that for stuffing.
constexpr long kEncBlockBytes = 2 * ((57 + 63 * 26 + 7) / 8) + 8;

long enc_intervals(const sv_jpeg_enc &p)
{
    const sv_jpeg_info &f = p.info;
    const long nmcu = (long)((f.width + 8 * f.h_samp - 1) / (8 * f.h_samp)) * ((f.height + 8 * f.v_samp - 1) / (8 * f.v_samp));
    return f.restart_interval > 0 ? (nmcu + f.restart_interval - 1) / f.restart_interval : 1;
}

long enc_bound(const sv_jpeg_enc &p, long values)
{
    const long blocks = p.info.coef_count / 64;
    return kEncHeaderMax + 2 * ((57 * blocks + 26 * values + 7) / 8) + 3 * enc_intervals(p) + 8;
}

// Bits go into a growing byte vector, most significant first; 0xFF is followed by a stuffed zero byte
struct BitSink {
    std::vector<uint8_t> buf;
    size_t pos = 0;
    uint64_t acc = 0;
    int n = 0;                                                     // bits held in acc, < 8 between calls

    inline void room(size_t bytes) { if (buf.size() - pos < bytes) buf.resize(std::max(buf.size() * 2, pos + bytes + 4096)); }
    inline void put(uint32_t bits, int len)                        // len <= 32; room() was called for what a block can take
    {
        acc = (acc << len) | bits;
        n += len;
        while (n >= 8) {
            const uint8_t b = (uint8_t)(acc >> (n - 8));
            buf[pos++] = b;
            if (b == 0xFF) buf[pos++] = 0;
            n -= 8;
        }
    }
    inline void pad() { if (n) put((1u << (8 - n)) - 1, 8 - n); acc = 0; }
    inline void raw(uint8_t b) { buf[pos++] = b; }
};

inline int bit_size(int v) { const unsigned a = (unsigned)(v < 0 ? -v : v); return a ? 32 - __builtin_clz(a) : 0; }

// Restart intervals [k0, k1) of a frame -> sink.  Returns SV_OK or SV_ERR_BAD_ARG (message set) for records no baseline file can hold.
int encode_intervals(const sv_jpeg_enc &p, const uint64_t *masks, const uint32_t *offsets, const int16_t *values, long values_count, long k0, long k1, BitSink &sink)
{
    const sv_jpeg_info &f = p.info;
    const EncTables &T = enc_tables();
    const int mcu_cols = (f.width + 8 * f.h_samp - 1) / (8 * f.h_samp), mcu_rows = (f.height + 8 * f.v_samp - 1) / (8 * f.v_samp);
    const long nmcu = (long)mcu_cols * mcu_rows, per = f.restart_interval > 0 ? f.restart_interval : nmcu;
    int ch[3], cv[3], bw[3];
    long boff[3], off = 0;
    for (int c = 0; c < f.components; c++) {
        ch[c] = c == 0 ? f.h_samp : 1; cv[c] = c == 0 ? f.v_samp : 1;
        bw[c] = mcu_cols * ch[c];
        boff[c] = off;
        off += (long)bw[c] * mcu_rows * cv[c];
    }
    for (long k = k0; k < k1; k++) {
        if (k > 0) { sink.room(2); sink.raw(0xFF); sink.raw((uint8_t)(0xD0 + ((k - 1) & 7))); }
        int pred[3] = {0, 0, 0};
        const long m1 = std::min(nmcu, (k + 1) * per);
        for (long mi = k * per; mi < m1; mi++) {
            const int mx = (int)(mi % mcu_cols), my = (int)(mi / mcu_cols);
            for (int c = 0; c < f.components; c++) {
                const EncCodes &dct = T.dc[c > 0], &act = T.ac[c > 0];
                for (int v = 0; v < cv[c]; v++)
                    for (int u = 0; u < ch[c]; u++) {
                        const long bi = boff[c] + (long)(my * cv[c] + v) * bw[c] + (mx * ch[c] + u);
                        const uint64_t mask = masks[bi];
                        const long first = (long)offsets[bi];
                        if (first + __builtin_popcountll(mask) > values_count)
                            return sv_fail(SV_ERR_BAD_ARG, "jpeg encode: block %ld refers to values beyond values_count %ld", bi, values_count);
                        const int16_t *val = values + first;
                        sink.room((size_t)kEncBlockBytes);
                        const int dc = (mask & 1) ? *val++ : 0;
                        if ((mask & 1) && dc == 0) return sv_fail(SV_ERR_BAD_ARG, "jpeg encode: block %ld has a zero value under a set mask bit", bi);
                        const int diff = dc - pred[c];
                        pred[c] = dc;
                        int size = bit_size(diff);
                        if (size > 11) return sv_fail(SV_ERR_BAD_ARG, "jpeg encode: block %ld: DC difference %d has no baseline code", bi, diff);
                        sink.put(dct.code[size], dct.len[size]);
                        if (size) sink.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << size) - 1), size);
                        uint64_t rest = mask >> 1;
                        int pos = 0;                               // zigzag position of the last coefficient coded
                        while (rest) {
                            int run = __builtin_ctzll(rest);
                            rest = (rest >> run) >> 1;
                            pos += run + 1;
                            const int a = *val++;
                            size = bit_size(a);
                            if (size == 0 || size > 10) return sv_fail(SV_ERR_BAD_ARG, "jpeg encode: block %ld: AC value %d has no baseline code", bi, a);
                            for (; run > 15; run -= 16) sink.put(act.code[0xF0], act.len[0xF0]);
                            const int sym = run << 4 | size;
                            sink.put(act.code[sym] << size | ((uint32_t)(a < 0 ? a - 1 : a) & ((1u << size) - 1)), act.len[sym] + size);
                        }
                        if (pos < 63) sink.put(act.code[0], act.len[0]);
                    }
            }
        }
        sink.pad();
    }
    return SV_OK;
}

size_t write_header(const sv_jpeg_enc &p, uint8_t *o)
{
    const sv_jpeg_info &f = p.info;
    uint8_t *s = o;
    auto seg = [&](int marker, int payload) { *o++ = 0xFF; *o++ = (uint8_t)marker; *o++ = (uint8_t)((payload + 2) >> 8); *o++ = (uint8_t)(payload + 2); };
    *o++ = 0xFF; *o++ = 0xD8;
    seg(0xE0, 14);
    const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    memcpy(o, jfif, 14); o += 14;
    for (int t = 0; t < (f.components == 3 ? 2 : 1); t++) {
        seg(0xDB, 65);
        *o++ = (uint8_t)t;
        for (int i = 0; i < 64; i++) *o++ = (uint8_t)p.quant[64 * t + kNatural[i]];
    }
    seg(0xC0, 6 + 3 * f.components);
    *o++ = 8; *o++ = (uint8_t)(f.height >> 8); *o++ = (uint8_t)f.height; *o++ = (uint8_t)(f.width >> 8); *o++ = (uint8_t)f.width; *o++ = (uint8_t)f.components;
    for (int c = 0; c < f.components; c++) { *o++ = (uint8_t)(c + 1); *o++ = (uint8_t)(c == 0 ? f.h_samp << 4 | f.v_samp : 0x11); *o++ = (uint8_t)(c > 0); }
    const struct { int id; const uint8_t *bits, *vals; int n; } dht[4] = {{0x00, kDcLumaBits, kDcVals, 12}, {0x10, kAcLumaBits, kAcLumaVals, 162},
                                                                         {0x01, kDcChromaBits, kDcVals, 12}, {0x11, kAcChromaBits, kAcChromaVals, 162}};
    for (int t = 0; t < (f.components == 3 ? 4 : 2); t++) {
        seg(0xC4, 17 + dht[t].n);
        *o++ = (uint8_t)dht[t].id;
        memcpy(o, dht[t].bits, 16); o += 16;
        memcpy(o, dht[t].vals, (size_t)dht[t].n); o += dht[t].n;
    }
    if (f.restart_interval) { seg(0xDD, 2); *o++ = (uint8_t)(f.restart_interval >> 8); *o++ = (uint8_t)f.restart_interval; }
    seg(0xDA, 4 + 2 * f.components);
    *o++ = (uint8_t)f.components;
    for (int c = 0; c < f.components; c++) { *o++ = (uint8_t)(c + 1); *o++ = (uint8_t)(c == 0 ? 0x00 : 0x11); }
    *o++ = 0; *o++ = 63; *o++ = 0;
    return (size_t)(o - s);
}

bool enc_plan_ok(const sv_jpeg_enc *p)
{
    if (!p) return false;
    const sv_jpeg_info &f = p->info;
    return f.width > 0 && f.height > 0 && f.width < 65536 && f.height < 65536 && (f.components == 1 || f.components == 3) &&
           ((f.h_samp == 1 && f.v_samp == 1) || (f.components == 3 && f.h_samp == 2 && (f.v_samp == 1 || f.v_samp == 2))) && f.restart_interval >= 0 &&
           f.restart_interval < 65536 && f.coef_count > 0;
}

int entropy_encode(const sv_jpeg_enc &p, const uint64_t *masks, const uint32_t *offsets, const int16_t *values, long values_count, uint8_t *out, size_t out_cap,
                   size_t *out_size, int threads)
{
    const long intervals = enc_intervals(p);
    const int chunks = (int)std::max(1L, std::min((long)threads, intervals));
    std::vector<BitSink> sinks((size_t)chunks);
    std::vector<int> rcs((size_t)chunks, SV_OK);
    std::vector<std::string> msgs((size_t)chunks);
    WorkerPool::instance().parallel_for(chunks, chunks, [&](int c) {
        rcs[c] = encode_intervals(p, masks, offsets, values, values_count, intervals * c / chunks, intervals * (c + 1) / chunks, sinks[c]);
        if (rcs[c]) msgs[c] = sv_last_error();                     // the message lives on the worker's thread
    });
    for (int c = 0; c < chunks; c++)
        if (rcs[c]) return sv_fail(rcs[c], "%s", msgs[c].c_str());
    uint8_t head[kEncHeaderMax];
    const size_t hn = write_header(p, head);
    size_t total = hn + 2;
    for (const BitSink &s : sinks) total += s.pos;
    *out_size = total;
    if (total > out_cap) return sv_fail(SV_ERR_BUFFER, "jpeg encode: the file takes %zu bytes, the buffer holds %zu", total, out_cap);
    memcpy(out, head, hn);
    size_t at = hn;
    for (const BitSink &s : sinks) { if (s.pos) memcpy(out + at, s.buf.data(), s.pos); at += s.pos; }
    out[at++] = 0xFF; out[at++] = 0xD9;
    return SV_OK;
}

}  // namespace

extern "C" int sv_jpeg_encode_plan(int width, int height, int components, int sampling, int quality, int restart, sv_jpeg_enc *plan)
{
    if (!plan) return sv_fail(SV_ERR_BAD_ARG, "sv_jpeg_encode_plan: NULL argument");
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535) return sv_fail(SV_ERR_BAD_ARG, "sv_jpeg_encode_plan: size %d x %d (1..65535)", width, height);
    if (components != 1 && components != 3) return sv_fail(SV_ERR_BAD_ARG, "sv_jpeg_encode_plan: %d components (1 or 3)", components);
    if (components == 3 && sampling != SV_JPEG_444 && sampling != SV_JPEG_422 && sampling != SV_JPEG_420)
        return sv_fail(SV_ERR_BAD_ARG, "sv_jpeg_encode_plan: unknown sampling %d", sampling);
    if (quality < 1 || quality > 100) return sv_fail(SV_ERR_BAD_ARG, "sv_jpeg_encode_plan: quality %d (1..100)", quality);
    if (restart < 0 || restart > 65535) return sv_fail(SV_ERR_BAD_ARG, "sv_jpeg_encode_plan: restart interval %d (0..65535)", restart);
    memset(plan, 0, sizeof *plan);
    sv_jpeg_info &f = plan->info;
    f.width = f.out_width = width; f.height = f.out_height = height;
    f.components = components;
    f.h_samp = components == 3 && sampling != SV_JPEG_444 ? 2 : 1;
    f.v_samp = components == 3 && sampling == SV_JPEG_420 ? 2 : 1;
    f.orientation = 1;
    f.restart_interval = restart;
    const long mcu_cols = (width + 8 * f.h_samp - 1) / (8 * f.h_samp), mcu_rows = (height + 8 * f.v_samp - 1) / (8 * f.v_samp);
    f.coef_count = 64 * mcu_cols * mcu_rows * (components == 3 ? f.h_samp * f.v_samp + 2 : 1);
    f.sparse_capacity = f.coef_count;
    plan->quality = quality;
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;       // jpeg_quality_scaling
    for (int c = 0; c < 3; c++)
        for (int i = 0; i < 64; i++) {
            const int q = std::min(255, std::max(1, ((c == 0 ? kBaseLuma[i] : kBaseChroma[i]) * scale + 50) / 100));
            plan->quant[64 * c + i] = (uint16_t)q;
            plan->recip[64 * c + i] = (uint32_t)(((1ull << 32) + 8 * q - 1) / (8 * q));
        }
    plan->out_bound = enc_bound(*plan, f.coef_count);
    return SV_OK;
}

extern "C" long sv_jpeg_encode_bound(const sv_jpeg_enc *plan, long values_count)
{
    if (!enc_plan_ok(plan) || values_count < 0) return -1;
    return enc_bound(*plan, std::min(values_count, plan->info.coef_count));
}

extern "C" int sv_jpeg_entropy_encode(const sv_jpeg_enc *plan, const uint64_t *masks, const uint32_t *offsets, const int16_t *values, long values_count, uint8_t *out,
                                      size_t out_cap, size_t *out_size, int threads)
{
    if (!plan || !masks || !offsets || !values || !out || !out_size) return sv_fail(SV_ERR_BAD_ARG, "sv_jpeg_entropy_encode: NULL argument");
    if (!enc_plan_ok(plan) || values_count < 0) return sv_fail(SV_ERR_BAD_ARG, "sv_jpeg_entropy_encode: bad plan or values_count");
    return entropy_encode(*plan, masks, offsets, values, values_count, out, out_cap, out_size, threads < 1 ? 1 : threads);
}

// Images of a batch over the pool's threads; every image packs its restart intervals serially (a worker's nested parallel_for runs inline)
extern "C" int sv_jpeg_entropy_encode_batch(const sv_jpeg_enc *plan, int n, const uint64_t *const *masks, const uint32_t *const *offsets, const int16_t *const *values,
                                            const long *values_count, uint8_t *const *outs, const size_t *out_caps, size_t *out_sizes, int threads, int *status)
{
    if (!plan || !masks || !offsets || !values || !values_count || !outs || !out_caps || !out_sizes || !status || n <= 0)
        return sv_fail(SV_ERR_BAD_ARG, "sv_jpeg_entropy_encode_batch: bad argument");
    if (!enc_plan_ok(plan)) return sv_fail(SV_ERR_BAD_ARG, "sv_jpeg_entropy_encode_batch: bad plan");
    if (threads < 1) threads = 1;
    auto one = [&](int i, int inner) {
        out_sizes[i] = 0;
        const bool ok = masks[i] && offsets[i] && values[i] && outs[i] && values_count[i] >= 0;
        status[i] = ok ? entropy_encode(*plan, masks[i], offsets[i], values[i], values_count[i], outs[i], out_caps[i], out_sizes + i, inner) : SV_ERR_BAD_ARG;
    };
    if (threads == 1 || n == 1) for (int i = 0; i < n; i++) one(i, n == 1 ? threads : 1);
    else WorkerPool::instance().parallel_for(n, threads, [&](int i) { one(i, 1); });
    for (int i = 0; i < n; i++)
        if (status[i] != SV_OK) return sv_fail(status[i], "sv_jpeg_entropy_encode_batch: image %d failed (see status[])", i);
    return SV_OK;
}
