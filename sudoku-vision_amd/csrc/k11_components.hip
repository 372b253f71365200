// K11: component filter -- a second exact accelerator for the HOST corner search (cv/grid.py:37-71), behind K4, not a reference stage.
//
// Definition (include/sudoku_vision_hip.h, sv_component_filter_u8): with min_area = min_area_ratio * ((double)H * (double)W), every
// 8-connected foreground component whose pixel bounding box x0..x1, y0..y1 has (double)(x1 - x0) * (double)(y1 - y0) < min_area is erased;
// every other pixel is unchanged.  No iteration cap, no "left as it is" case.
// Why it is exact: find_grid_contour skips a contour whose bounding-box product is under the floor (host_contours.cpp, grid_corners_from),
// and a contour's area never exceeds that product, so an erased component can never be a candidate; Suzuki-Abe only looks at the
// 8-neighbours of the component being traced, so erasing one changes no other border; a traced small component leaves the scan's
// outside-state as it found it; and a component nested in a hole of a kept one is not external either way.  This is K4's argument
// (top of k4_despeckle.hip) with "strictly inside a tile" replaced by "bounding box under the floor", hence
//     find_grid_contour(filter(b, r), r') == find_grid_contour(b, r')   for every r' >= r.
//
// The work is done on the 1-bit image (LSB = leftmost, wpr words per row) and on RUNS, not pixels.  A run start is a foreground pixel
// whose left neighbour is background: starts = w & ~((w << 1) | carry), carry = bit 31 of the previous word of the row.  The k-th run start
// of row y gets slot y * rowcap + k with rowcap = 16 * wpr (a row of 32 * wpr pixels holds at most that many runs), so slots are in raster
// order, a slot tells its row, and only a scan along each row is needed to number them.  Phases, one launch each (a launch boundary is the
// only hand-off between them):
//   1 k_cc_scan      wave per row: base[y][k] = slot of the first run start of word k; parent[slot] = slot; the slot's box is emptied
//   2 k_cc_union     thread per word: every piece of a run inside the word is united with every run of the row above that touches the
//                    piece's columns widened by one (8-connectivity).  Lock-free union-find: find both roots, atomicMin the smaller root
//                    into the larger one's parent word, and if that word had meanwhile changed go on with what it held.  A parent is
//                    always a smaller slot, so the trees have no cycles and a component's root is its first run in raster order.
//   3 k_cc_compress  thread per word: every run start points at its root
//   4 k_cc_box       thread per word: every piece does atomicMin / atomicMax on its root's x0, x1, y1 (y0 is the root's own row)
//   5 k_cc_erase     thread per word: the criterion, in double and as written above, per piece; what is kept of the word goes to base[]
//   6 k_cc_store / k_cc_mask   the kept words into the bit image in place, or the byte image masked by them
// Visibility (per-XCD L2s are not coherent with each other, and a CU's L1 is never refreshed by another CU's stores): inside the launches
// that write them (2, 3) every access to a parent word is a relaxed agent-scope atomic (load, fetch_min, store), never a plain access;
// the boxes are only written in 4 (agent-scope atomics without return) and only read in 5.  Everything else is read-only within a launch.
// The result depends only on the partition into components -- roots are minima, boxes are min/max -- never on the order the atomics land in.
//
// Scratch (sv_ctx::cc, grow-only), per frame of H x W with wpr = ceil(W / 32):  4 * H * wpr bytes of `base`, 4 arrays of 4 * H * 16 * wpr
// bytes (parent, x0, x1, y1: one word per possible run start; only the words of runs that exist are touched), and for the byte entry
// another 4 * H * wpr for the bit image: 264 (bits entry: 260) bytes per 32 pixels, i.e. 8.25 B per pixel reserved, of which a photo
// touches a few per cent.  Batches are cut into groups of frames so that the scratch stays under CC_SCRATCH_CAP where one frame fits.
#include "sv_device.h"
#include "sv_internal.h"

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr size_t CC_SCRATCH_CAP = (size_t)1 << 30;

struct cc_frame {          // per-group scratch arrays; frame f's part starts at f * (words or slots per frame)
    u32 *base, *parent, *x0, *x1, *y1;
};

__device__ __forceinline__ u32 ld_parent(const u32 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ u32 find_root(const u32 *parent, u32 x)
{
    for (;;) {
        const u32 p = ld_parent(parent + x);
        if (p == x) return x;
        x = p;
    }
}

__device__ __forceinline__ void unite(u32 *parent, u32 a, u32 b)
{
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        if (a < b) { const u32 t = a; a = b; b = t; }                      // a: the larger root, to hang under b
        const u32 old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;                                               // a was still a root: linked
        a = old;                                                            // a had been linked elsewhere meanwhile: unite that with b
    }
}

// the lowest run of ones in m: its mask
__device__ __forceinline__ u32 lowest_run(u32 m) { const u32 low = m & (0u - m); return ((m + low) ^ m) & m; }
__device__ __forceinline__ u64 lowest_run(u64 m) { const u64 low = m & (0ull - m); return ((m + low) ^ m) & m; }

// slot of the run that holds bit s of word w (s set in w): `starts` the word's run starts, `base` the slot of its first one.  A piece
// that begins at bit 0 as the continuation of a run gets base - 1, the last start before this word, which is that run's.
__device__ __forceinline__ u32 slot_of(u32 base, u32 starts, int s) { return base - 1 + (u32)__popc(starts & (u32)((2ull << s) - 1)); }

// ---- 1: number the run starts of every row, initialise their slots ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cc_scan(const u32 *__restrict__ bits, int H, int wpr, long rows, cc_frame fr)
{
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int y = (int)(row % H);
    const long frame = row / H;
    const u32 rowcap = 16u * (u32)wpr;
    const u32 *brow = bits + row * wpr;
    u32 *base = fr.base + row * wpr;
    const size_t so = (size_t)frame * H * rowcap;                         // the frame's first slot
    u32 running = (u32)y * rowcap, carry = 0;                              // carry: bit 31 of the word before this chunk
    for (int k0 = 0; k0 < wpr; k0 += 64) {
        const int k = k0 + lane;
        const u32 w = k < wpr ? brow[k] : 0u;
        u32 prev = __shfl_up(w, 1);
        if (lane == 0) prev = carry;
        const u32 starts = w & ~((w << 1) | (prev >> 31));
        const u32 c = (u32)__popc(starts);
        u32 incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u32 v = __shfl_up(incl, d);
            if (lane >= d) incl += v;
        }
        const u32 b = running + incl - c;
        if (k < wpr) base[k] = b;
        u32 m = starts, i = 0;
        while (m) {
            const size_t s = so + b + i;
            fr.parent[s] = b + i;
            fr.x0[s] = 0xFFFFFFFFu;
            fr.x1[s] = 0u;
            fr.y1[s] = 0u;
            m &= m - 1;
            i++;
        }
        running += __shfl(incl, 63);
        carry = __shfl(w, 63);
    }
}

// ---- 2: unite the runs of row y with those of row y - 1 ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cc_union(const u32 *__restrict__ bits, int H, int wpr, long words, cc_frame fr)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= words) return;
    const int k = (int)(idx % wpr);
    const long row = idx / wpr;
    const int y = (int)(row % H);
    if (y == 0) return;
    const u32 cur = bits[idx];
    if (!cur) return;
    const u32 *up = bits + idx - wpr;
    const u64 U = (k > 0 ? (u64)(up[-1] >> 31) : 0ull) | ((u64)up[0] << 1) | (k + 1 < wpr ? (u64)(up[1] & 1u) << 33 : 0ull);   // bit j = column 32k + j - 1
    if (!U) return;
    const long frame = row / H;
    u32 *parent = fr.parent + (size_t)frame * H * (16u * (size_t)wpr);
    const u32 carry = k > 0 ? bits[idx - 1] >> 31 : 0u;
    const u32 starts = cur & ~((cur << 1) | carry);
    const u32 cbase = fr.base[idx], ubase = fr.base[idx - wpr];
    const u64 T = (U & ~(U << 1)) & ~1ull;                                  // run starts of the row above at window bits 1..33
    u32 m = cur;
    while (m) {
        const u32 piece = lowest_run(m);
        m &= ~piece;
        const int s = __ffs((int)piece) - 1;
        const u64 wide = (u64)piece | ((u64)piece << 1) | ((u64)piece << 2);   // the piece's columns widened by one, in window bits
        u64 uw = U & wide;
        if (!uw) continue;
        const u32 a = slot_of(cbase, starts, s);
        while (uw) {
            const u64 q = lowest_run(uw);
            uw &= ~q;
            const int j = __ffsll((long long)q) - 1;
            const u32 b = ubase - 1 + (u32)__popcll(T & ((2ull << j) - 1));
            unite(parent, a, b);
        }
    }
}

// ---- 3: every run start points at its root ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cc_compress(const u32 *__restrict__ bits, int H, int wpr, long words, cc_frame fr)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= words) return;
    const u32 cur = bits[idx];
    if (!cur) return;
    const int k = (int)(idx % wpr);
    const long frame = idx / wpr / H;
    u32 *parent = fr.parent + (size_t)frame * H * (16u * (size_t)wpr);
    const u32 carry = k > 0 ? bits[idx - 1] >> 31 : 0u;
    const u32 n = (u32)__popc(cur & ~((cur << 1) | carry));
    const u32 b = fr.base[idx];
    for (u32 i = 0; i < n; i++) {
        const u32 r = find_root(parent, b + i);
        __hip_atomic_store(parent + b + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- 4: bounding boxes --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cc_box(const u32 *__restrict__ bits, int H, int wpr, long words, cc_frame fr)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= words) return;
    const u32 cur = bits[idx];
    if (!cur) return;
    const int k = (int)(idx % wpr);
    const long row = idx / wpr;
    const u32 y = (u32)(row % H);
    const size_t so = (size_t)(row / H) * H * (16u * (size_t)wpr);
    const u32 carry = k > 0 ? bits[idx - 1] >> 31 : 0u;
    const u32 starts = cur & ~((cur << 1) | carry);
    const u32 b = fr.base[idx];
    u32 m = cur;
    while (m) {
        const u32 piece = lowest_run(m);
        m &= ~piece;
        const int s = __ffs((int)piece) - 1, e = 31 - __clz((int)piece);
        const size_t r = so + fr.parent[so + slot_of(b, starts, s)];
        __hip_atomic_fetch_min(fr.x0 + r, (u32)(32 * k + s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(fr.x1 + r, (u32)(32 * k + e), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(fr.y1 + r, y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- 5: the criterion ---------------------------------------------------------------------------------------------------------------------
// What is left of word idx goes to base[idx], which only this thread reads in this launch: writing the image itself here would race with
// the neighbour to the right, which reads this word's bit 31 to tell its own run starts.
__global__ __launch_bounds__(256) void k_cc_erase(const u32 *__restrict__ bits, int H, int wpr, long words, cc_frame fr, double min_area)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= words) return;
    const u32 cur = bits[idx];
    if (!cur) { fr.base[idx] = 0u; return; }
    const int k = (int)(idx % wpr);
    const long row = idx / wpr;
    const u32 rowcap = 16u * (u32)wpr;
    const size_t so = (size_t)(row / H) * H * (size_t)rowcap;
    const u32 carry = k > 0 ? bits[idx - 1] >> 31 : 0u;
    const u32 starts = cur & ~((cur << 1) | carry);
    const u32 b = fr.base[idx];
    u32 m = cur, keep = cur;
    while (m) {
        const u32 piece = lowest_run(m);
        m &= ~piece;
        const int s = __ffs((int)piece) - 1;
        const u32 root = fr.parent[so + slot_of(b, starts, s)];
        const size_t r = so + root;
        const u32 y0 = root / rowcap;
        if ((double)(fr.x1[r] - fr.x0[r]) * (double)(fr.y1[r] - y0) < min_area) keep &= ~piece;
    }
    fr.base[idx] = keep;
}

// ---- 6: the result, as bits in place or as bytes ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cc_store(u32 *__restrict__ bits, const u32 *__restrict__ kept, long words)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= words) return;
    const u32 w = kept[idx];
    if (w != bits[idx]) bits[idx] = w;
}

// byte image -> padded bit rows (wpr = ceil(W / 32) words per row, the bits past W are zero)
__global__ __launch_bounds__(256) void k_cc_pack(const u8 *__restrict__ src, int W, int wpr, long words, u32 *__restrict__ bits)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= words) return;
    const int k = (int)(idx % wpr);
    const u8 *p = src + (idx / wpr) * (long)W + 32 * k;
    const int n = W - 32 * k < 32 ? W - 32 * k : 32;
    u32 w = 0;
    for (int i = 0; i < n; i++) w |= (u32)(p[i] != 0) << i;
    bits[idx] = w;
}

// out = binary where the pixel is kept, 0 elsewhere (out may be binary); packed (W % 32 == 0 only): the kept bits as well
__global__ __launch_bounds__(256) void k_cc_mask(const u8 *__restrict__ src, const u32 *__restrict__ kept, int W, int wpr, long words, u8 *__restrict__ dst,
                                                 u32 *__restrict__ packed)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= words) return;
    const int k = (int)(idx % wpr);
    const long o = (idx / wpr) * (long)W + 32 * k;
    const int n = W - 32 * k < 32 ? W - 32 * k : 32;
    const u32 w = kept[idx];
    if (packed) packed[idx] = w;
    for (int i = 0; i < n; i++) dst[o + i] = (w >> i) & 1 ? src[o + i] : (u8)0;
}

inline unsigned blocks(long items, int per) { return (unsigned)((items + per - 1) / per); }

}  // namespace

// bits: n frames of H rows of wpr words (read only).  What the filter keeps of them is left in fr.base, word for word.
// min_area is the floor itself (the entries compute it from the true frame size).
static int cc_filter_group(const cc_frame &fr, const u32 *bits, int n, int H, int wpr, double min_area, hipStream_t s)
{
    const long rows = (long)n * H, words = rows * wpr;
    hipLaunchKernelGGL(k_cc_scan, dim3(blocks(rows, 4)), dim3(256), 0, s, bits, H, wpr, rows, fr);
    SV_LAUNCH_CHECK("k_cc_scan");
    hipLaunchKernelGGL(k_cc_union, dim3(blocks(words, 256)), dim3(256), 0, s, bits, H, wpr, words, fr);
    SV_LAUNCH_CHECK("k_cc_union");
    hipLaunchKernelGGL(k_cc_compress, dim3(blocks(words, 256)), dim3(256), 0, s, bits, H, wpr, words, fr);
    SV_LAUNCH_CHECK("k_cc_compress");
    hipLaunchKernelGGL(k_cc_box, dim3(blocks(words, 256)), dim3(256), 0, s, bits, H, wpr, words, fr);
    SV_LAUNCH_CHECK("k_cc_box");
    hipLaunchKernelGGL(k_cc_erase, dim3(blocks(words, 256)), dim3(256), 0, s, bits, H, wpr, words, fr, min_area);
    SV_LAUNCH_CHECK("k_cc_erase");
    return SV_OK;
}

// Frames per group and the scratch a group needs: base + 4 slot arrays (+ the bit image) per frame.
static int cc_plan(sv_ctx *ctx, int n, int H, int wpr, bool own_bits, int *group, size_t *frame_words)
{
    const size_t fw = (size_t)H * wpr, per_frame = fw * 4 * (1 + 4 * 16 + (own_bits ? 1 : 0));
    size_t g = CC_SCRATCH_CAP / per_frame;
    g = g < 1 ? 1 : (g > (size_t)n ? (size_t)n : g);
    *group = (int)g;
    *frame_words = fw;
    return ctx->cc.grow(ctx, g * per_frame);
}

static cc_frame cc_layout(sv_ctx *ctx, int group, size_t fw)
{
    u32 *p = ctx->cc.as<u32>();
    const size_t slots = (size_t)group * fw * 16;
    cc_frame fr;
    fr.base = p;
    fr.parent = p + (size_t)group * fw;
    fr.x0 = fr.parent + slots;
    fr.x1 = fr.x0 + slots;
    fr.y1 = fr.x1 + slots;
    return fr;
}

int svk_component_filter_bits(sv_ctx *ctx, uint32_t *bits, int n, int H, int W, double min_area, hipStream_t s)
{
    const int wpr = W >> 5;
    int group;
    size_t fw;
    int rc = cc_plan(ctx, n, H, wpr, false, &group, &fw);
    if (rc) return rc;
    const cc_frame fr = cc_layout(ctx, group, fw);
    for (int f = 0; f < n; f += group) {
        const int m = n - f < group ? n - f : group;
        const long words = (long)m * H * wpr;
        u32 *b = bits + (size_t)f * fw;
        rc = cc_filter_group(fr, b, m, H, wpr, min_area, s);
        if (rc) return rc;
        hipLaunchKernelGGL(k_cc_store, dim3(blocks(words, 256)), dim3(256), 0, s, b, fr.base, words);
        SV_LAUNCH_CHECK("k_cc_store");
    }
    return SV_OK;
}

int svk_component_filter(sv_ctx *ctx, const u8 *binary, int n, int H, int W, double min_area, u8 *out, uint32_t *packed, hipStream_t s)
{
    const int wpr = (W + 31) >> 5;
    int group;
    size_t fw;
    int rc = cc_plan(ctx, n, H, wpr, true, &group, &fw);
    if (rc) return rc;
    const cc_frame fr = cc_layout(ctx, group, fw);
    u32 *own = fr.y1 + (size_t)group * fw * 16;                             // the bit image, behind the slot arrays
    for (int f = 0; f < n; f += group) {
        const int m = n - f < group ? n - f : group;
        const long words = (long)m * H * wpr;
        const u8 *src = binary + (size_t)f * H * W;
        hipLaunchKernelGGL(k_cc_pack, dim3(blocks(words, 256)), dim3(256), 0, s, src, W, wpr, words, own);
        SV_LAUNCH_CHECK("k_cc_pack");
        rc = cc_filter_group(fr, own, m, H, wpr, min_area, s);
        if (rc) return rc;
        hipLaunchKernelGGL(k_cc_mask, dim3(blocks(words, 256)), dim3(256), 0, s, src, fr.base, W, wpr, words, out + (size_t)f * H * W,
                           packed ? packed + (size_t)f * fw : (u32 *)nullptr);
        SV_LAUNCH_CHECK("k_cc_mask");
    }
    return SV_OK;
}
