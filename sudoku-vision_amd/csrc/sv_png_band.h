// One band of a PNG image -> its piece of the deflate stream (k18_png_encode.hip).  The band's work is written as phases: phase(tid) is what
// thread tid of the 256 does between two workgroup barriers, reads only what earlier phases wrote and shares nothing with the other threads of
// its own phase but atomic adds / ors.  The kernel runs the phases with __syncthreads() in between; a host program can run them as plain loops
// over tid (tools/dev/png_encode_asan.cpp does, under AddressSanitizer: every index below is checked there before it meets a GPU).
//
// Band = band_rows whole rows of filtered bytes (filter-type byte + W * bpp bytes a row), at most kMaxBandBytes, so that one stored block holds it.
//   filter     rows are filtered from ORIGINAL neighbours (global memory; the row above a band's first row is the image's, zero above row 0), so
//              bands do not depend on each other.  BGR is swapped to RGB here.  adaptive: per row the filter with the smallest
//              sum of abs((int8) byte), the lowest number on a tie.
//   tokens     Z_RLE: a maximal run of k equal bytes is one literal, then matches of distance 1 and length min(258, rest) while the rest is >= 3,
//              then literals.  Position 0 starts a run: no match reaches back across the band's first byte.  Thread t owns the tokens that START
//              in its chunk of ceil(bytes / 256) bytes; the run a chunk starts or ends inside is found from the per-chunk first / last run starts.
//   code       histogram of the 286 literal/length symbols (+ end of block) -> rank sort by (count, symbol) -> one lane builds the Huffman tree with
//              two queues, limits the lengths to 15 bits (moving leaves down until the Kraft sum is 1) and hands out canonical codes.
//   block      BFINAL 0, BTYPE 2, HLIT, HDIST = 2 codes (lengths 1, 1: complete whatever the band holds), HCLEN 19 with the constant code-length code
//              "0..15: 4 bits, 16 / 17 / 18 unused", the lengths 4 bits each, the tokens, end of block, then an empty stored block (pad, 00 00 FF FF):
//              the band ends on a byte.  When that is no smaller than one stored block (5 + bytes) the band is the stored block.
//   adler      Adler-32 of the band's filtered bytes (start value 1); the host combines the bands'.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SVP_HD __host__ __device__ inline
#else
#define SVP_HD inline
#endif

namespace svpng {

constexpr int kThreads = 256;
constexpr int kMaxRows = 512;            // rows of a band: the adaptive filter's row sums live in LDS
constexpr int kMaxBandBytes = 65535;     // one stored block
constexpr int kSmallBandBytes = 35000;   // two such workgroups share a CU's 160 KiB (static_assert below)
constexpr int kSyms = 286, kEob = 256;
constexpr uint32_t kAdlerBase = 65521;
enum { kFilterAdaptive = 5 };
enum { kRle = 0, kHuffmanOnly = 1, kStored = 2 };

struct Geom {
    int W, H, bpp;                       // bpp 1 (gray) or 3 (BGR in, RGB out)
    int filter, strategy;
    int band_rows, bands, row_bytes;     // row_bytes = 1 + W * bpp
    long pitch, frame_stride, slot_bytes;
};

// per-thread values that live from one phase to the next
struct Lane { int rs_in, re_in; uint32_t bit_at; };

template <class T> SVP_HD void atomic_add(T *p, T v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
SVP_HD void atomic_or(uint32_t *p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, v);
#else
    *p |= v;
#endif
}

SVP_HD int paeth(int a, int b, int c)
{
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}
SVP_HD uint8_t filter_byte(int f, int x, int a, int b, int c)
{
    return (uint8_t)(f == 0 ? x : f == 1 ? x - a : f == 2 ? x - b : f == 3 ? x - ((a + b) >> 1) : x - paeth(a, b, c));
}
// match length 3..258 -> length code 0..28 (symbol 257 + code), its extra bits and their value
SVP_HD void length_code(int len, int &code, int &ebits, int &evalue)
{
    const int l = len - 3;
    if (len == 258) { code = 28; ebits = 0; evalue = 0; return; }
    if (l < 8) { code = l; ebits = 0; evalue = 0; return; }
    int msb = 3;
    while ((l >> (msb + 1)) != 0) msb++;
    ebits = msb - 2;
    code = 4 * ebits + 4 + ((l >> ebits) & 3);
    evalue = l & ((1 << ebits) - 1);
}
SVP_HD uint32_t bit_reverse(uint32_t v, int n)
{
    uint32_t r = 0;
    for (int i = 0; i < n; i++) { r = (r << 1) | (v & 1); v >>= 1; }
    return r;
}

template <int CAP>
struct Band {
    static constexpr int kOutWords = CAP / 4 + 8;
    uint8_t fb[(CAP + 15) / 16 * 16];    // the filtered band
    uint32_t out[kOutWords];             // the packed block; before that the adaptive filter's row sums [rows][5]
    uint32_t hist[288];
    uint16_t order[288], code[288], parent[576];
    union { uint32_t key[288]; uint32_t nfreq[576]; };                // the sort keys are done with (phase 7) when the tree's counts are written (phase 8)
    union { struct { uint32_t ad_a[kThreads], ad_b[kThreads]; }; uint16_t depth[576]; };   // the chunks' Adler sums are folded (phase 5) before the tree is walked
    uint8_t len[288], rfilt[kMaxRows];
    int blast[kThreads], bfirst[kThreads];
    uint32_t tbits[kThreads];
    int nbytes, rows, y0, chunk, hlit, coded;
    uint32_t adler, out_bytes;
    static_assert(kMaxRows * 5 <= kOutWords, "the row sums borrow the output words");

    SVP_HD int raw(const Geom &g, const uint8_t *img, int y, int x) const
    {
        if (y < 0 || x < 0) return 0;
        const int px = g.bpp == 3 ? x / 3 : x, ch = x - px * g.bpp;
        return img[(long)y * g.pitch + (long)px * g.bpp + (g.bpp == 3 ? 2 - ch : 0)];
    }

    // ---- phase 0: geometry of this band, cleared counters
    SVP_HD void p0_init(const Geom &g, int band, int tid)
    {
        if (tid == 0) {
            y0 = band * g.band_rows;
            rows = g.H - y0 < g.band_rows ? g.H - y0 : g.band_rows;
            nbytes = rows * g.row_bytes;
            chunk = (nbytes + kThreads - 1) / kThreads;
            hlit = 257; coded = 0; adler = 1; out_bytes = 0;
        }
        for (int i = tid; i < 288; i += kThreads) { hist[i] = i == kEob ? 1u : 0u; len[i] = 0; code[i] = 0; }
        const int r = g.H - band * g.band_rows < g.band_rows ? g.H - band * g.band_rows : g.band_rows;
        for (int i = tid; i < r; i += kThreads) rfilt[i] = (uint8_t)(g.filter == kFilterAdaptive ? 0 : g.filter);
        if (g.filter == kFilterAdaptive)
            for (int i = tid; i < r * 5; i += kThreads) out[i] = 0;
    }
    // ---- phase 1 (adaptive): sums of abs((int8) byte) of every filter, 32 bytes of a row at a time
    SVP_HD void p1_row_sums(const Geom &g, const uint8_t *img, int tid)
    {
        const int rb = g.row_bytes - 1, per_row = (rb + 31) / 32;
        for (int item = tid; item < rows * per_row; item += kThreads) {
            const int r = item / per_row, x0 = (item - r * per_row) * 32, x1 = x0 + 32 < rb ? x0 + 32 : rb, y = y0 + r;
            uint32_t s[5] = {0, 0, 0, 0, 0};
            for (int x = x0; x < x1; x++) {
                const int v = raw(g, img, y, x), a = raw(g, img, y, x - g.bpp), b = raw(g, img, y - 1, x), c = x >= g.bpp ? raw(g, img, y - 1, x - g.bpp) : 0;
                for (int f = 0; f < 5; f++) {
                    const int e = (int8_t)filter_byte(f, v, a, b, c);
                    s[f] += (uint32_t)(e < 0 ? -e : e);
                }
            }
            for (int f = 0; f < 5; f++) atomic_add(&out[r * 5 + f], s[f]);
        }
    }
    // ---- phase 2 (adaptive): the row's filter
    SVP_HD void p2_row_choice(int tid)
    {
        for (int r = tid; r < rows; r += kThreads) {
            int best = 0;
            for (int f = 1; f < 5; f++)
                if (out[r * 5 + f] < out[r * 5 + best]) best = f;
            rfilt[r] = (uint8_t)best;
        }
    }
    // ---- phase 3: the filtered bytes; the output words are cleared for the packer
    SVP_HD void p3_filter(const Geom &g, const uint8_t *img, int tid)
    {
        for (int i = tid; i < kOutWords; i += kThreads) out[i] = 0;
        for (int i = tid; i < nbytes; i += kThreads) {
            const int r = i / g.row_bytes, c = i - r * g.row_bytes, f = rfilt[r];
            if (c == 0) { fb[i] = (uint8_t)f; continue; }
            const int x = c - 1, y = y0 + r;
            const int v = raw(g, img, y, x);
            int a = 0, b = 0, cc = 0;
            if (f == 1 || f >= 3) a = raw(g, img, y, x - g.bpp);
            if (f >= 2) b = raw(g, img, y - 1, x);
            if (f == 4 && x >= g.bpp) cc = raw(g, img, y - 1, x - g.bpp);
            fb[i] = filter_byte(f, v, a, b, cc);
        }
    }
    SVP_HD bool run_starts(int i) const { return i == 0 || fb[i] != fb[i - 1]; }
    // ---- phase 4: first and last run start of every chunk; the chunk's Adler sums
    SVP_HD void p4_chunks(int tid)
    {
        const int c0 = tid * chunk < nbytes ? tid * chunk : nbytes, c1 = c0 + chunk < nbytes ? c0 + chunk : nbytes;
        int first = nbytes, last = -1;
        uint32_t a = 0, b = 0;
        for (int i = c0; i < c1; i++) {
            if (run_starts(i)) { if (first == nbytes) first = i; last = i; }
            a += fb[i];
            b += (uint32_t)(c1 - i) * fb[i];
        }
        bfirst[tid] = first; blast[tid] = last; ad_a[tid] = a; ad_b[tid] = b; tbits[tid] = 0;
    }
    // The tokens that start in thread tid's chunk, in order: f.literal(byte), f.match(length)
    template <class F> SVP_HD void walk(const Geom &g, const Lane &L, int tid, F &f) const
    {
        const int c0 = tid * chunk < nbytes ? tid * chunk : nbytes, c1 = c0 + chunk < nbytes ? c0 + chunk : nbytes;
        if (g.strategy == kHuffmanOnly) {
            for (int p = c0; p < c1; p++) f.literal(fb[p]);
            return;
        }
        if (c0 >= c1) return;
        int rs = run_starts(c0) ? c0 : L.rs_in;
        for (int p = c0; p < c1;) {
            int e = p + 1;
            while (e < c1 && fb[e] == fb[e - 1]) e++;
            const int re = e < c1 ? e : L.re_in;                    // the next run start, in this chunk or a later one
            const int m = re - rs - 1, stop = re < c1 ? re : c1;     // m bytes follow the run's first
            while (p < stop) {
                const int j = p - rs;
                if (j == 0 || m < 3) { f.literal(fb[p]); p++; continue; }
                const int q = (j - 1) / 258, r = (j - 1) - q * 258, mq = m - q * 258 < 258 ? m - q * 258 : 258;
                if (mq < 3) { f.literal(fb[p]); p++; }
                else if (r == 0) { f.match(mq); p += mq; }
                else p += mq - r;                                    // inside a match that started in an earlier chunk
            }
            rs = re;
        }
    }
    struct Count {
        uint32_t *hist;
        SVP_HD void literal(int b) { atomic_add(&hist[b], 1u); }
        SVP_HD void match(int n) { int c, eb, ev; length_code(n, c, eb, ev); atomic_add(&hist[257 + c], 1u); }
    };
    struct Measure {
        const uint8_t *len; uint32_t bits;
        SVP_HD void literal(int b) { bits += len[b]; }
        SVP_HD void match(int n) { int c, eb, ev; length_code(n, c, eb, ev); bits += (uint32_t)(len[257 + c] + eb + 1); }
    };
    SVP_HD void put(uint32_t pos, uint32_t v, int n)
    {
        (void)n;
        const uint64_t x = (uint64_t)v << (pos & 31);
        const uint32_t w = pos >> 5;
        if (w + 1 >= (uint32_t)kOutWords) return;                    // cannot happen: the block is smaller than the stored band
        atomic_or(&out[w], (uint32_t)x);
        if (x >> 32) atomic_or(&out[w + 1], (uint32_t)(x >> 32));
    }
    struct Emit {
        Band *b; uint32_t pos;
        SVP_HD void literal(int s) { b->put(pos, b->code[s], b->len[s]); pos += b->len[s]; }
        SVP_HD void match(int n)
        {
            int c, eb, ev;
            length_code(n, c, eb, ev);
            const int l = b->len[257 + c];
            b->put(pos, (uint32_t)b->code[257 + c] | (uint32_t)ev << l, l + eb + 1);         // the distance code (symbol 0: distance 1) is one 0 bit
            pos += (uint32_t)(l + eb + 1);
        }
    };
    // ---- phase 5: the run a chunk starts and ends inside; histogram; thread 0 folds the chunks' Adler sums
    SVP_HD void p5_histogram(const Geom &g, Lane &L, int tid)
    {
        int rs = 0, re = nbytes;
        for (int j = 0; j < kThreads; j++) {
            if (j < tid && blast[j] > rs) rs = blast[j];
            if (j > tid && bfirst[j] < re) re = bfirst[j];
        }
        L.rs_in = rs; L.re_in = re; L.bit_at = 0;
        if (tid == 0) {
            uint32_t A = 1, B = 0;
            for (int j = 0; j < kThreads; j++) {
                const int c0 = j * chunk < nbytes ? j * chunk : nbytes, c1 = c0 + chunk < nbytes ? c0 + chunk : nbytes;
                B = (B + (uint32_t)(c1 - c0) * A + ad_b[j]) % kAdlerBase;
                A = (A + ad_a[j]) % kAdlerBase;
            }
            adler = B << 16 | A;
        }
        if (g.strategy == kStored) return;
        Count f{hist};
        walk(g, L, tid, f);
    }
    // ---- phase 6, 7: sort keys (count, symbol), unused symbols last; every symbol's rank
    SVP_HD void p6_keys(int tid)
    {
        for (int s = tid; s < 288; s += kThreads) key[s] = s < kSyms && hist[s] ? hist[s] << 9 | (uint32_t)s : 0xffffffffu;
    }
    SVP_HD void p7_rank(int tid)
    {
        for (int s = tid; s < kSyms; s += kThreads) {
            const uint32_t k = key[s];
            if (k == 0xffffffffu) continue;
            int rank = 0;
            for (int j = 0; j < kSyms; j++) rank += key[j] < k;
            order[rank] = (uint16_t)s;
        }
    }
    // ---- phase 8: one lane: tree, lengths of at most 15 bits, canonical codes (bit-reversed: deflate sends Huffman codes most significant bit first)
    SVP_HD void p8_code(int tid)
    {
        if (tid != 0) return;
        int n = 0;
        for (int s = 0; s < kSyms; s++) n += hist[s] != 0;          // >= 2: a band has a literal, and the end of block
        for (int i = 0; i < n; i++) nfreq[i] = hist[order[i]];
        int li = 0, ih = n, it = n;
        for (int k = 0; k + 1 < n; k++) {
            int pick[2];
            for (int u = 0; u < 2; u++) pick[u] = li < n && (ih >= it || nfreq[li] <= nfreq[ih]) ? li++ : ih++;
            nfreq[it] = nfreq[pick[0]] + nfreq[pick[1]];
            parent[pick[0]] = parent[pick[1]] = (uint16_t)it;
            it++;
        }
        int count[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        depth[it - 1] = 0;
        for (int i = it - 2; i >= 0; i--) {
            depth[i] = (uint16_t)(depth[parent[i]] + 1);
            if (i < n) count[depth[i] < 15 ? depth[i] : 15]++;
        }
        uint32_t total = 0;
        for (int i = 15; i > 0; i--) total += (uint32_t)count[i] << (15 - i);
        while (total > (1u << 15)) {                                  // too deep a tree was cut at 15: move leaves down until the code is complete again
            count[15]--;
            for (int i = 14; i > 0; i--)
                if (count[i]) { count[i]--; count[i + 1] += 2; break; }
            total--;
        }
        int j = n;
        for (int l = 1; l <= 15; l++)
            for (int c = count[l]; c > 0; c--) len[order[--j]] = (uint8_t)l;
        uint32_t next[16], c = 0;
        next[0] = 0;
        for (int l = 1; l <= 15; l++) { c = (c + (uint32_t)(l > 1 ? count[l - 1] : 0)) << 1; next[l] = c; }
        int last = 256;
        for (int s = 0; s < kSyms; s++)
            if (len[s]) { code[s] = (uint16_t)bit_reverse(next[len[s]]++, len[s]); if (s > last) last = s; }
        hlit = last + 1;
    }
    // ---- phase 9: bits of every chunk's tokens
    SVP_HD void p9_measure(const Geom &g, const Lane &L, int tid)
    {
        Measure f{len, 0};
        walk(g, L, tid, f);
        tbits[tid] = f.bits;
    }
    // ---- phase 10: coded or stored; the coded block into the output words
    SVP_HD void p10_pack(const Geom &g, Lane &L, int tid)
    {
        uint32_t before = 0, all = 0;
        for (int j = 0; j < kThreads; j++) { before += j < tid ? tbits[j] : 0; all += tbits[j]; }
        const uint32_t head = 17 + 57 + 4 * (uint32_t)(hlit + 2);
        const uint32_t end = head + all + len[kEob] + 3;             // + the empty stored block's BFINAL and BTYPE
        const uint32_t bytes = (end + 7) / 8 + 4;
        const bool is_coded = g.strategy != kStored && bytes < (uint32_t)nbytes + 5;
        if (tid == 0) { coded = is_coded; out_bytes = is_coded ? bytes : (uint32_t)nbytes + 5; }
        if (!is_coded) return;
        for (int s = tid; s < hlit + 2; s += kThreads) put(74 + 4 * (uint32_t)s, bit_reverse(s < hlit ? len[s] : 1, 4), 4);
        if (tid == 0) {
            put(0, 0u | 2u << 1 | (uint32_t)(hlit - 257) << 3 | 1u << 8 | 15u << 13, 17);       // BFINAL 0, BTYPE 2, HLIT, HDIST 2 - 1, HCLEN 19 - 4
            // code lengths of the code-length code in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15: three 0, sixteen 4
            for (int i = 3; i < 19; i++) put(17 + 3 * (uint32_t)i, 4, 3);
            put(head + all, code[kEob], len[kEob]);
            put(((end + 7) / 8 + 2) * 8, 0xffffu, 16);               // LEN 0, NLEN ffff of the empty stored block
        }
        L.bit_at = head + before;
        Emit f{this, L.bit_at};
        walk(g, L, tid, f);
    }
    // ---- phase 11: the band's slot, length, Adler sum and status
    SVP_HD void p11_store(const Geom &g, uint8_t *slot, uint32_t *band_len, uint32_t *band_adler, uint32_t *status, int tid)
    {
        const bool fits = (long)out_bytes <= g.slot_bytes;
        if (tid == 0) { *band_len = fits ? out_bytes : 0; *band_adler = adler; *status = fits ? 0 : 1; }
        if (!fits) return;
        if (coded) {
            uint32_t *w = (uint32_t *)slot;                           // slots are 16-byte aligned and a multiple of 16 bytes
            for (uint32_t i = tid; i < (out_bytes + 3) / 4; i += kThreads) w[i] = out[i];
            return;
        }
        if (tid == 0) {
            slot[0] = 0;
            slot[1] = (uint8_t)nbytes; slot[2] = (uint8_t)(nbytes >> 8);
            slot[3] = (uint8_t)~nbytes; slot[4] = (uint8_t)(~nbytes >> 8);
        }
        for (int i = tid; i < nbytes; i += kThreads) slot[5 + i] = fb[i];
    }
};

static_assert(sizeof(Band<kSmallBandBytes>) <= 80 * 1024 && sizeof(Band<kMaxBandBytes>) <= 160 * 1024, "LDS: two small bands or one large band a CU");

}  // namespace svpng
