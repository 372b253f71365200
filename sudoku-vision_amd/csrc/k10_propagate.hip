// K10 -- run_v2's constraint propagation (pipeline/run_v2.py:373-391: resolve_with_constraints, pipeline/constraint_resolver.py:48-267,
// ConstraintResolver.__init__ + propagate) for n frames in one launch, every field equal to the reference's (DESIGN.md "K10").
//
//   k_propagate : one wave (a 64-thread workgroup) per frame.  A lane owns cells `lane` and `lane + 64`: their values and their
//   candidates (a mask, bit d = d possible) stay in its registers from the first read to the last write.
//     init      per digit two ballots give the 81-bit mask of the cells showing it; a cell loses every digit one of its peers shows,
//               filled cells too (two peers showing one digit leave each other without candidates, which nothing ever reports).
//     a pass    the naked singles, found by ballot, listed in cell order, then placed one after the other; then the hidden singles:
//               per digit the ballots of "shows it" and "empty and may take it", and lanes 0..26 (one unit each, rows, columns, boxes)
//               see whether their unit lacks the digit and has one place for it -- the reference's list, (unit, digit) order, with
//               each entry's tuple hash; lane 0 replays CPython's set on that list (set_order) and the wave places the entries in the
//               order the set hands them back; then the first empty cell without candidates ends the frame.
//   Placing is the wave's: the entry is uniform, the owner's lane answers "filled?" and "still a candidate?" through ballots, and
//   every lane takes the digit from those of its cells that are peers.  No array is indexed by a run-time value in registers;
//   everything that is lives in LDS.
//
// Order rules (all from the reference): naked singles are found before any is placed, and one whose digit an earlier one of the same
// pass took is the contradiction; hidden singles are found after the naked ones are placed, and are placed in the order of
// list(set(list)): an entry whose cell was filled earlier in the pass is skipped, one whose digit is gone is the contradiction.
// The set: CPython 3.8+'s tuple hash (xxHash-style, 64 bits) of (row, col, digit) and Objects/setobject.c's table: 8 slots at first,
// slot i and (where they all fit) the 9 after it, then i = 5 i + 1 + (perturb >>= 5); an entry that brings it to fill * 5 >= mask * 3
// grows it to the smallest power of two above 4 * used, old entries re-inserted in slot order.  A pass has at most 27 * 9 entries,
// so the table never passes 512 slots.
#include "sv_device.h"
#include "sv_internal.h"
#include "sv_m81.h"

namespace {

constexpr int PENT = 27 * 9;          // hidden singles of a pass before deduplication, at most
constexpr int PTAB = 512;             // slots of the set's table, at most (77..243 distinct entries)
constexpr uint32_t PFREE = 0xFFFF;    // a free slot
constexpr uint32_t PNONE = 255;       // no contradiction cell; an unused entry of `resolved`
constexpr uint32_t PALL = 0x3FE;      // candidates 1..9

struct Smem {
    uint64_t hash[PENT];              // hash((row, col, digit)) of the pass's hidden singles, list order
    uint16_t ent[PENT];               // the entries themselves: cell << 4 | digit
    uint16_t tab[2][PTAB];            // the set's table: entry numbers; the second is what it grows into
    uint16_t order[PENT];             // entries in the order they are placed in
    uint16_t res[81];                 // cells_resolved
    int next, used, grow;             // lane 0's account of its insertions
};

struct Cells {
    int v[2];                         // the lane's two cells (the second only for lane < 17): value
    uint32_t c[2];                    //                                                       candidates
};

__device__ __forceinline__ uint64_t tuple_hash3(uint32_t a, uint32_t b, uint32_t c)
{
    constexpr uint64_t P1 = 11400714785074694791ull, P2 = 14029467366897019727ull, P5 = 2870177450012600261ull;
    uint64_t acc = P5;
    const uint32_t item[3] = {a, b, c};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        acc += item[i] * P2;
        acc = (acc << 31) | (acc >> 33);
        acc *= P1;
    }
    acc += 3ull ^ (P5 ^ 3527539ull);
    return acc == ~0ull ? 1546275796ull : acc;
}

// The slot an entry of hash h goes to: the first free one on its probe path, or -1 when the path meets an entry equal to `key` first
// (key < 0: the table holds none).  One lane.  The path reaches every slot once perturb has run out, within 13 + PTAB rounds.
__device__ int probe(const uint16_t *tab, const uint16_t *ent, uint32_t mask, uint64_t h, int key)
{
    uint64_t perturb = h;
    uint32_t i = (uint32_t)h & mask;
    for (int round = 0; round < 13 + PTAB + 1; round++) {
        const uint32_t n = i + 9 <= mask ? 10 : 1;
        for (uint32_t j = 0; j < n; j++) {
            const uint32_t t = tab[i + j];
            if (t == PFREE) return (int)(i + j);
            if (key >= 0 && ent[min(t, (uint32_t)PENT - 1)] == key) return -1;
        }
        perturb >>= 5;
        i = (i * 5 + 1 + (uint32_t)perturb) & mask;
    }
    return -1;
}

// list(set(S.ent[0..total))) -> S.order, returns how many.  Lane 0 inserts; the wave clears tables and reads the result off.
__device__ int set_order(Smem &S, int total, int lane)
{
    const uint64_t below = (1ull << lane) - 1;
    int cur = 0;
    uint32_t mask = 7;
    if (lane < 8) S.tab[0][lane] = (uint16_t)PFREE;
    if (lane == 0) { S.next = 0; S.used = 0; }
    for (int growth = 0; growth < 4; growth++) {                      // 8 -> 32 -> 128 -> 512 slots
        __syncthreads();
        if (lane == 0) {
            uint16_t *tab = S.tab[cur];
            int e = S.next, used = S.used, grow = 0;
            while (e < total && !grow) {
                const int slot = probe(tab, S.ent, mask, S.hash[e], S.ent[e]);
                if (slot >= 0) {
                    tab[slot] = (uint16_t)e;
                    used++;
                    grow = (uint32_t)used * 5 >= mask * 3;
                }
                e++;
            }
            S.next = e; S.used = used; S.grow = grow;
        }
        __syncthreads();
        if (!S.grow) break;
        uint32_t size = 8;
        while (size <= (uint32_t)S.used * 4 && size < PTAB) size <<= 1;
        for (uint32_t i = lane; i < size; i += 64) S.tab[cur ^ 1][i] = (uint16_t)PFREE;
        __syncthreads();
        if (lane == 0) {
            for (uint32_t i = 0; i <= mask; i++) {
                const uint32_t t = S.tab[cur][i];
                if (t == PFREE) continue;
                const int slot = probe(S.tab[cur ^ 1], S.ent, size - 1, S.hash[min(t, (uint32_t)PENT - 1)], -1);
                if (slot >= 0) S.tab[cur ^ 1][slot] = (uint16_t)t;
            }
        }
        cur ^= 1;
        mask = size - 1;
    }
    __syncthreads();
    int n = 0;
    for (uint32_t base = 0; base <= mask; base += 64) {               // the table from slot 0 up
        const uint32_t t = base + lane <= mask ? S.tab[cur][base + lane] : PFREE;
        const uint64_t votes = __ballot(t != PFREE);
        if (t != PFREE) S.order[min(n + (int)__popcll(votes & below), PENT - 1)] = S.ent[min(t, (uint32_t)PENT - 1)];
        n += __popcll(votes);
    }
    __syncthreads();
    return min(n, PENT);
}

// _set_cell(x, d) by the whole wave (x, d uniform) -> 0 placed, 1 the cell is filled already, 2 d is not among its candidates
__device__ __forceinline__ int place(Cells &C, int lane, int x, int d)
{
    const int s = x >> 6;
    const bool mine = lane == (x & 63);
    const int v = s ? C.v[1] : C.v[0];
    const uint32_t c = s ? C.c[1] : C.c[0];
    if (__ballot(mine && v != 0)) return 1;
    if (!__ballot(mine && (c >> d & 1))) return 2;
    const int r = x / 9, col = x % 9, b = box_of(x);
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int y = lane + 64 * t;
        if (y != x && (y / 9 == r || y % 9 == col || box_of(y) == b)) C.c[t] &= ~(1u << d);   // y > 80: a cell nobody reads
        if (mine && s == t) { C.v[t] = d; C.c[t] = 1u << d; }
    }
    return 0;
}

struct PropOut { u8 *grid; uint16_t *cand; u8 *valid; int *iterations; u8 *bad; u8 *nres; u8 *res; u8 *fixed; };

__global__ __launch_bounds__(64) void k_propagate(const u8 *digits, const float *conf, int max_it, PropOut out)
{
    __shared__ Smem S;
    const int lane = threadIdx.x;
    const long f = blockIdx.x;
    const uint64_t below = (1ull << lane) - 1;
    const bool has1 = lane < 81 - 64;

    Cells C;
    C.v[0] = digits[f * 81 + lane];
    C.v[1] = has1 ? digits[f * 81 + 64 + lane] : 0;
    if (out.fixed) {
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const int x = lane + 64 * s;
            if (x < 81) out.fixed[f * 81 + x] = (u8)(C.v[s] > 0 && (conf ? (double)conf[f * 81 + x] : 1.0) > 0.9);
        }
    }

    int it = 0, nres = 0;
    uint32_t bad = PNONE;
    const bool grid_ok = !__ballot(C.v[0] > 9 || C.v[1] > 9);        // a byte that is no digit: reported invalid, nothing is computed
    C.c[0] = C.c[1] = 0;
    if (grid_ok) {
        // ---- __init__: every filled cell takes its value from its peers -----------------------------------------------------------
        m81 peers[2];
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const int x = min(lane + 64 * s, 80);
            const m81 u = row_mask(x / 9) | col_mask(x % 9) | box_mask(box_of(x));
            peers[s] = u & ~shl({1, 0}, x);
            C.c[s] = C.v[s] ? 1u << C.v[s] : PALL;
        }
#pragma unroll
        for (int d = 1; d <= 9; d++) {
            const m81 shown = {__ballot(C.v[0] == d), __ballot(has1 && C.v[1] == d)};
#pragma unroll
            for (int s = 0; s < 2; s++)
                if (any(shown & peers[s])) C.c[s] &= ~(1u << d);
        }

        // ---- propagate ------------------------------------------------------------------------------------------------------------
        while (it < max_it) {
            it++;
            bool progress = false;
            // naked singles: all found, then placed in cell order
            const bool nk0 = C.v[0] == 0 && __popc(C.c[0]) == 1, nk1 = has1 && C.v[1] == 0 && __popc(C.c[1]) == 1;
            const uint64_t b0 = __ballot(nk0), b1 = __ballot(nk1);
            if (nk0) S.order[__popcll(b0 & below)] = (uint16_t)(lane << 4 | (__ffs((int)C.c[0]) - 1));
            if (nk1) S.order[__popcll(b0) + __popcll(b1 & below)] = (uint16_t)((lane + 64) << 4 | (__ffs((int)C.c[1]) - 1));
            __syncthreads();
            int n = __popcll(b0) + __popcll(b1);
            for (int i = 0; i < n && bad == PNONE; i++) {
                const uint32_t e = __builtin_amdgcn_readfirstlane(S.order[i]);
                if (place(C, lane, e >> 4, e & 15)) { bad = e >> 4; break; }
                if (lane == 0 && nres < 81) S.res[nres] = (uint16_t)e;
                nres++;
                progress = true;
            }
            if (bad != PNONE) break;
            __syncthreads();

            // hidden singles on the new state: lane u < 27 looks at unit u, digits ascending
            const m81 unit = unit_mask(min(lane, 26));
            uint32_t hit = 0, where[10];
#pragma unroll
            for (int d = 1; d <= 9; d++) {
                const m81 shown = {__ballot(C.v[0] == d), __ballot(has1 && C.v[1] == d)};
                const m81 open = {__ballot(C.v[0] == 0 && (C.c[0] >> d & 1)), __ballot(has1 && C.v[1] == 0 && (C.c[1] >> d & 1))};
                const m81 spots = open & unit;
                where[d] = (uint32_t)first(spots) & 127;
                if (lane < 27 && !any(shown & unit) && pop(spots) == 1) hit |= 1u << d;
            }
            const int mine = __popc(hit);
            int upto = mine;
#pragma unroll
            for (int o = 1; o < 32; o <<= 1) {                        // units are lanes 0..26: a scan over 32 lanes
                const int t = __shfl_up(upto, o);
                if (lane >= o) upto += t;
            }
            const int total = __shfl(upto, 26);
            int at = upto - mine;
#pragma unroll
            for (int d = 1; d <= 9; d++) {
                if (hit >> d & 1) {
                    const int q = min(at, PENT - 1);
                    S.ent[q] = (uint16_t)(where[d] << 4 | d);
                    S.hash[q] = tuple_hash3(where[d] / 9, where[d] % 9, d);
                    at++;
                }
            }
            n = set_order(S, total, lane);
            for (int i = 0; i < n; i++) {
                const uint32_t e = __builtin_amdgcn_readfirstlane(S.order[i]);
                const int rc = place(C, lane, e >> 4, e & 15);
                if (rc == 1) continue;                                // filled earlier in this pass
                if (rc == 2) { bad = e >> 4; break; }
                if (lane == 0 && nres < 81) S.res[nres] = (uint16_t)e;
                nres++;
                progress = true;
            }
            if (bad != PNONE) break;
            // the first empty cell left without candidates
            const m81 dead = {__ballot(C.v[0] == 0 && C.c[0] == 0), __ballot(has1 && C.v[1] == 0 && C.c[1] == 0)};
            if (any(dead)) { bad = first(dead); break; }
            if (!progress) break;
            __syncthreads();
        }
    }
    __syncthreads();

    // ---- outputs ------------------------------------------------------------------------------------------------------------------
    nres = min(nres, 81);
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const int x = lane + 64 * s;
        if (x < 81) {
            const long o = f * 81 + x;
            if (out.grid) out.grid[o] = (u8)C.v[s];
            if (out.cand) out.cand[o] = (uint16_t)C.c[s];
            if (out.res) {
                const uint32_t e = x < nres ? S.res[x] : 0;
                out.res[2 * o] = (u8)(x < nres ? e >> 4 : PNONE);
                out.res[2 * o + 1] = (u8)(x < nres ? e & 15 : PNONE);
            }
        }
    }
    if (lane == 0) {
        if (out.valid) out.valid[f] = (u8)(grid_ok && bad == PNONE);
        if (out.iterations) out.iterations[f] = it;
        if (out.bad) out.bad[f] = (u8)bad;
        if (out.nres) out.nres[f] = (u8)nres;
    }
}

}  // namespace

int svk_propagate_constraints(const u8 *digits, const float *conf, long n, int max_iterations, u8 *grid, uint16_t *candidates, u8 *is_valid, int *iterations,
                              u8 *contradiction_cell, u8 *n_resolved, u8 *resolved, u8 *is_fixed, hipStream_t s)
{
    const PropOut out = {grid, candidates, is_valid, iterations, contradiction_cell, n_resolved, resolved, is_fixed};
    hipLaunchKernelGGL(k_propagate, dim3((unsigned)n), dim3(64), 0, s, digits, conf, max_iterations, out);
    SV_LAUNCH_CHECK("k_propagate");
    return SV_OK;
}
